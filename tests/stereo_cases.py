"""Directed cases for Frame::ComputeStereoMatches by feature injection.

A stereo case is a pair of real pyramids (extracted from real images) whose keypoints,
descriptors and counts are then replaced by crafted ones, so that the matcher alone runs on
inputs that hit the reference's decision edges on purpose (src/Frame.cc:496-686): Hamming
distances of exactly 74 / 75 / 99 / 100, equal-distance candidates, uR == minU and uR == maxU
and one float32 step beyond, the first and last row of the band [floor(y - 2s), ceil(y + 2s)]
and one row beyond, octaves levelL +- 1 against +- 2, the disparity <= 0 clamp, empty views
and a full kp_cap.  One extraction per base image serves every case.

THE INVARIANT.  Neither the reference, the oracle nor k_stereo bounds its window reads, so
every injected keypoint keeps what the extractor guarantees: octave in [0, nlevels), at
least BORDER pixels from every edge of its own level (in that level's coordinates) and, for
a right keypoint, floor(y - 2s) >= 0 and ceil(y + 2s) <= H - 1.  `check_invariant` asserts it
on every case before `generate` returns: a violation would be an out-of-bounds read on the
GPU, not a test failure.

Everything is deterministic in the seed.  The generator reports the directed constructs it
planted (`Case.constructs`: name -> left keypoint indices); it derives them from its own
candidate arithmetic (band, octave, [minU, maxU], Hamming distance), never from a matcher's
result.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from my_orb_slam2_amd import synth
from my_orb_slam2_amd._lib import KEYPOINT_DTYPE

F = np.float32
PARAMS = (500, 1.2, 8, 20, 7)
SIZE = (361, 150)                      # width, height of the base images
MBF = 386.1448
# maxD = mbf / mb = 70.3 px: [minU, maxU] then has both ends inside a 361-pixel image (the
# datasets' maxD, fx = 718.856, would put minU left of every image here)
MB = float(F(MBF) / F(70.3))
BORDER = 16
# kp_cap of a 361 x 150 handle with PARAMS: sum over the levels of features_per_level + 3
# (the GPU test asserts the library agrees)
KP_CAP = 524
# pair counts of the GPU regime test, in its order, and the workgroups per pair of each
REGIMES = (16, 129, 33, 1, 128, 17, 65, 32, 64)
SPLIT = {1: 16, 16: 16, 17: 8, 32: 8, 33: 4, 64: 4, 65: 2, 128: 2, 129: 1}
SPECIAL = ("left_empty", "right_empty", "both_empty", "one_each", "full_cap")
N_SITES = 16
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def pair_seed(B: int, p: int) -> int:
    return 7919 * B + 31 * p + 5


def pair_kind(B: int, p: int) -> str:
    """The last five pairs of a batch are the special ones (a one-pair batch has none)."""
    return SPECIAL[p - (B - 5)] if B > 5 and p >= B - 5 else "regular"


def hamming(a, b):
    """[len(a), len(b)] Hamming distances of two (n, 32) uint8 descriptor arrays."""
    if len(a) == 0 or len(b) == 0:
        return np.zeros((len(a), len(b)), np.int32)
    ba = np.unpackbits(a, axis=1).astype(np.float32)
    bb = np.unpackbits(b, axis=1).astype(np.float32)
    return (ba.sum(1)[:, None] + bb.sum(1)[None, :] - 2.0 * (ba @ bb.T)).astype(np.int32)


def level_sizes(width, height, inv_scale):
    """ComputePyramid's level sizes (src/ORBextractor.cc:1133-1134: cvRound of float products)."""
    return [(int(np.rint(F(width) * F(s))), int(np.rint(F(height) * F(s)))) for s in inv_scale]


def band(y, octave, scale):
    """(minr, maxr) of right keypoints (src/Frame.cc:525-527), float32 as there."""
    y = np.asarray(y, F)
    r = (F(2.0) * np.asarray(scale, F)[octave]).astype(F)
    return np.floor((y - r).astype(F)).astype(np.int64), np.ceil((y + r).astype(F)).astype(np.int64)


def invariant_ok(k, sizes, scale, inv_scale, right):
    """Per keypoint: the invariant of the module docstring."""
    n = len(k)
    if n == 0:
        return np.zeros(0, bool)
    o = k["octave"].astype(np.int64)
    ok = (o >= 0) & (o < len(sizes))
    oc = np.clip(o, 0, len(sizes) - 1)
    lw = np.array([s[0] for s in sizes])[oc]
    lh = np.array([s[1] for s in sizes])[oc]
    inv = np.asarray(inv_scale, F)[oc]
    for v, lim in ((k["x"], lw), (k["y"], lh)):
        lv = (v.astype(F) * inv).astype(F)          # the level coordinate the SAD rounds
        rl = np.copysign(np.floor(np.abs(lv) + F(0.5)), lv)
        ok &= np.isfinite(lv) & (lv >= BORDER) & (lv <= lim - 1 - BORDER)
        ok &= (rl >= BORDER) & (rl <= lim - 1 - BORDER)
    if right:
        mn, mx = band(k["y"], oc, scale)
        ok &= (mn >= 0) & (mx <= sizes[0][1] - 1)
    else:
        ok &= (k["y"] >= 0) & (k["y"].astype(np.int64) < sizes[0][1])
    return ok


def check_invariant(kL, kR, sizes, scale, inv_scale):
    assert invariant_ok(kL, sizes, scale, inv_scale, False).all(), "left keypoint breaks the border invariant"
    assert invariant_ok(kR, sizes, scale, inv_scale, True).all(), "right keypoint breaks the border invariant"


# ---- base pairs ------------------------------------------------------------------------------
def _sad_sites(levels, scale, inv_scale, rng, count):
    """Keypoints at pixels of one image whose 11 x 11 window (Frame.cc:601-631, the image
    against itself) has SAD 0 at the centre only and equal SADs one pixel left and right: the
    parabola's deltaR is then exactly 0, the disparity exactly 0, and Frame.cc:659-663 clamps
    it.  Keypoints the extractor finds almost never sit on such a pixel (0 - 1 per image)."""
    out = []
    for o in range(3):
        P = levels[o].astype(np.int32)
        h, w = P.shape
        ys, xs = np.mgrid[19:h - 19, 19:w - 19]

        def sad(inc):
            D = P - np.roll(P, -inc, axis=1)          # D[y, x] = P[y, x] - P[y, x + inc]
            s = np.zeros(ys.shape, np.int64)
            for j in range(-5, 6):
                for i in range(-5, 6):
                    s += np.abs(D[ys + j, xs + i] - D[ys, xs])
            return s
        s = {inc: sad(inc) for inc in (-5, -4, -3, -2, -1, 1)}
        good = (s[-1] == s[1]) & (s[-1] > 0)
        for inc in (-5, -4, -3, -2):
            good &= s[inc] > 0
        for y, x in zip(ys[good], xs[good]):
            kx, ky = F(F(x) * F(scale[o])), F(F(y) * F(scale[o]))
            if np.floor(F(kx * F(inv_scale[o])) + F(0.5)) == x and np.floor(F(ky * F(inv_scale[o])) + F(0.5)) == y:
                out.append((kx, ky, o))
    pick = rng.permutation(len(out))[:count]
    k = np.zeros(len(pick), KEYPOINT_DTYPE)
    for n, i in enumerate(pick):
        k[n] = (out[i][0], out[i][1], 31.0 * scale[out[i][2]], 0.0, 1.0, out[i][2], -1)
    return k, rng.integers(0, 256, (len(pick), 32), dtype=np.uint8)


def base_pairs(oracle_mod):
    """The four base pairs: synth.stereo_pair(60 + i, 361, 150); in pair 0 the right image is
    the left image (zero scene disparity, SAD 0 at the centre) and both views carry the extra
    `_sad_sites` keypoints, whose self-match takes the disparity <= 0 clamp.  Each base keeps
    its two oracle extractors (pyramids extracted once; `set_features` swaps the features)."""
    bases = []
    for i in range(4):
        L, R = synth.stereo_pair(60 + i, *SIZE)
        if i == 0:
            R = L
        ol, orr = oracle_mod.OracleExtractor(*PARAMS), oracle_mod.OracleExtractor(*PARAMS)
        kL, dL = ol(L)
        kR, dR = orr(R)
        tab = ol.tables()
        b = dict(index=i, imgL=L, imgR=R, ol=ol, orr=orr, scale=tab["scale"], inv_scale=tab["inv_scale"],
                 sizes=level_sizes(SIZE[0], SIZE[1], tab["inv_scale"]), same=i == 0, n_sites=0)
        assert b["sizes"] == [ol.level_size(l) for l in range(PARAMS[2])]
        if i == 0:
            ks, ds = _sad_sites([ol.level(l) for l in range(3)], tab["scale"], tab["inv_scale"],
                                np.random.default_rng(600), N_SITES)
            b["n_sites"] = len(ks)
            kL, dL = np.concatenate([kL, ks]), np.concatenate([dL, ds])
            kR, dR = kL.copy(), dL.copy()
        b.update(kL=kL, dL=dL, kR=kR, dR=dR, ham=hamming(dL, dR))
        bases.append(b)
    return bases


# ---- one case --------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    kL: np.ndarray
    dL: np.ndarray
    kR: np.ndarray
    dR: np.ndarray
    kind: str
    base: int
    constructs: dict


def _flip(rng, desc, k, start=None):
    """Copies of the (n, 32) descriptors with exactly k[i] distinct bits flipped: k[i]
    consecutive entries, from start[i], of one random order of the 256 bits."""
    n = len(desc)
    rank = rng.permutation(256)
    start = rng.integers(0, 256, n) if start is None else np.asarray(start)
    mask = ((rank[None, :] - start[:, None]) % 256) < np.asarray(k)[:, None]
    return desc ^ np.packbits(mask.astype(np.uint8), axis=1)


def _clone_xy(rng, kL, idx, octave, xkind, ykind, scale, maxD):
    """Right-keypoint coordinates of clones of left keypoints `idx` at octaves `octave`.
    xkind 0: uR == maxU (zero disparity), 1: one float32 step above maxU, 2: uR == minU,
    3: one step below minU, 4: anywhere inside.  ykind 0 / 1: int(vL) is the band's first /
    last row, 2 / 3: one row before the first / after the last, 4: inside; on the half-pixel
    grid, or (one in four) at the float32 value nearest the exact edge."""
    n = len(idx)
    uL, vL = kL["x"][idx].astype(F), kL["y"][idx].astype(F)
    minU = (uL - F(maxD)).astype(F)
    x = np.where(xkind == 0, uL, np.where(xkind == 1, np.nextafter(uL, F(np.inf)),
        np.where(xkind == 2, minU, np.where(xkind == 3, np.nextafter(minU, F(-np.inf)),
        (uL - rng.uniform(0.5, maxD - 0.5, n).astype(F)).astype(F))))).astype(F)
    row = vL.astype(np.int64).astype(np.float64)
    r = (F(2.0) * np.asarray(scale, F)[octave]).astype(np.float64)
    t = rng.integers(0, 2, n)
    exact = rng.random(n) < 0.25
    m0 = np.ceil(2.0 * (row + r))
    m1 = np.floor(2.0 * (row - r))
    inside = np.rint(2.0 * (vL + rng.uniform(-1.0, 1.0, n) * np.maximum(r - 1.0, 0.0))) / 2.0
    y = np.select([ykind == 0, ykind == 1, ykind == 2, ykind == 3],
                  [np.where(exact, row + r, (m0 + t) / 2.0), np.where(exact, row - r, (m1 - t) / 2.0),
                   np.where(exact, row + 1.0 + r, (m0 + 2 + t) / 2.0),
                   np.where(exact, row - 1.0 - r, (m1 - 2 - t) / 2.0)], inside)
    return x, y.astype(F)


def _regular(base, rng, kp_cap, maxD):
    kL, dL, kR0, dR0 = base["kL"], base["dL"], base["kR"], base["dR"]
    scale, inv_scale, sizes = base["scale"], base["inv_scale"], base["sizes"]
    NL, nlev, H = len(kL), len(scale), sizes[0][1]
    rowL = kL["y"].astype(np.int64)
    levL = kL["octave"].astype(np.int64)
    site = np.zeros(NL, bool)
    if base["n_sites"]:
        site[NL - base["n_sites"]:] = True

    # rows that no right band may touch: their left keypoints find vRowIndices[row] empty
    ZW = 4
    cnt = np.convolve(np.bincount(rowL[~site], minlength=H), np.ones(ZW, np.int64))[ZW - 1:H - 1]
    a0 = int(rng.choice(np.nonzero(cnt >= min(7, cnt.max()))[0]))
    dead = (rowL >= a0) & (rowL < a0 + ZW)

    def off_zone(k):
        mn, mx = band(k["y"], k["octave"], scale)
        return (mx < a0) | (mn >= a0 + ZW)

    # roles of the left keypoints: 0 real candidates only, 1 one planted clone, 2 a tie group
    role = rng.choice(3, NL, p=[0.2, 0.66, 0.14])
    role[site | dead] = 0
    planted_k, planted_d, owner, tie_of, xkind_of = [], [], [], [], []

    def plant(idx, octave, xkind, ykind, nflip, x=None, start=None):
        cx, y = _clone_xy(rng, kL, idx, octave, xkind, ykind, scale, maxD)
        k = kL[idx].copy()
        k["x"], k["y"], k["octave"], k["class_id"] = cx if x is None else x, y, octave, -1
        k["size"] = (F(31.0) * np.asarray(scale, F)[octave]).astype(F)
        ok = invariant_ok(k, sizes, scale, inv_scale, True) & off_zone(k)
        return k, _flip(rng, dL[idx], nflip, start), ok

    # (b) clones, one per left keypoint: Hamming distance x column x row x octave
    idx = np.nonzero(role == 1)[0]
    n = len(idx)
    kk = rng.choice(6, n, p=[0.2, 0.17, 0.13, 0.13, 0.1, 0.27])
    nflip = np.select([kk == 0, kk == 1, kk == 2, kk == 3, kk == 4], [0, 74, 75, 99, 100],
                      rng.integers(1, 74, n))
    xkind = rng.choice(5, n, p=[0.17, 0.09, 0.17, 0.09, 0.48])
    ykind = rng.choice(5, n, p=[0.2, 0.2, 0.1, 0.1, 0.4])
    octave = np.clip(levL[idx] + rng.choice([-2, -1, 0, 1, 2], n, p=[0.08, 0.22, 0.4, 0.22, 0.08]),
                     0, nlev - 1)
    k, d, ok = plant(idx, octave, xkind, ykind, nflip)
    # a clone that would break the invariant is drawn again inside the range and the band, at
    # the left keypoint's own octave; one that still breaks it is left out
    bad = np.nonzero(~ok)[0]
    if len(bad):
        xkind[bad], ykind[bad], octave[bad] = 4, 4, levL[idx[bad]]
        k2, d2, ok2 = plant(idx[bad], octave[bad], xkind[bad], ykind[bad], nflip[bad])
        k[bad], d[bad], ok[bad] = k2, d2, ok2
    planted_k.append(k[ok]); planted_d.append(d[ok]); owner.append(idx[ok])
    tie_of.append(np.full(ok.sum(), -1))
    xkind_of.append(xkind[ok])

    # (c) tie groups: 2 - 3 clones of one left keypoint at the same distance, different bits,
    # columns more than two SAD search ranges apart where [minU, maxU] has the room (so the
    # wrong one changes uRight)
    groups = np.nonzero(role == 2)[0]
    if len(groups):
        size = rng.integers(2, 4, len(groups))
        ii = np.repeat(groups, size)
        gid = np.repeat(np.arange(len(groups)), size)
        member = np.arange(len(ii)) - np.repeat(np.cumsum(size) - size, size)
        kf = np.where(rng.random(len(groups)) < 0.5, 74, rng.integers(3, 70, len(groups)))[gid]
        # disparities: a random base plus a multiple of the separation, wrapped into the range
        sep = np.maximum(12.0 * np.asarray(scale, np.float64)[levL[ii]], (maxD - 2.0) / 3.5)
        ds = 1.0 + (rng.uniform(0.0, maxD - 2.0, len(groups))[gid] + member * sep) % (maxD - 2.0)
        octs = np.clip(levL[ii] + rng.integers(-1, 2, len(ii)), 0, nlev - 1)
        k, d, ok = plant(ii, octs, np.full(len(ii), 4), rng.choice([0, 1, 4], len(ii)), kf,
                         x=(kL["x"][ii] - ds.astype(F)).astype(F),
                         start=rng.integers(0, 256, len(groups))[gid] + 85 * member)
        planted_k.append(k[ok]); planted_d.append(d[ok]); owner.append(ii[ok])
        tie_of.append(gid[ok])
        xkind_of.append(np.full(ok.sum(), -1))
    pk, pd = np.concatenate(planted_k), np.concatenate(planted_d)
    own, tie = np.concatenate(owner), np.concatenate(tie_of)

    # (a) real right keypoints: out of the dead rows, and not a candidate below TH_HIGH of a
    # left keypoint that has planted clones (its outcome is then the planted one's)
    keep = off_zone(kR0)
    if base["same"]:
        # the image against itself: a kept right keypoint is its left twin's SAD-0 match.  Too
        # many of those make the median SAD 0, and the cut then removes every match
        keep &= (rng.random(len(kR0)) < 0.1) | site
    mnR, mxR = band(kR0["y"], kR0["octave"], scale)
    directed = np.nonzero(role > 0)[0]
    cand = ((mnR[None, :] <= rowL[directed, None]) & (mxR[None, :] >= rowL[directed, None]) &
            (np.abs(kR0["octave"][None, :].astype(np.int64) - levL[directed, None]) <= 1) &
            (base["ham"][directed] < 100))
    keep &= ~cand.any(axis=0)
    real = np.nonzero(keep)[0]
    room = kp_cap - len(pk)
    if len(real) > room:
        real = np.sort(rng.permutation(real)[:max(room, 0)])
    kR = np.concatenate([kR0[real], pk])
    dR = np.concatenate([dR0[real], pd])
    own = np.concatenate([np.full(len(real), -1), own])
    tie = np.concatenate([np.full(len(real), -1), tie])
    xk = np.concatenate([np.full(len(real), -1)] + xkind_of)
    # the right array is shuffled last: iR order is unrelated to row, octave or source
    perm = rng.permutation(len(kR))
    kR, dR, own, tie, xk = kR[perm], dR[perm], own[perm], tie[perm], xk[perm]
    return kL, dL, kR, dR, _constructs(kL, dL, kR, dR, own, tie, xk, scale, maxD)


def _constructs(kL, dL, kR, dR, own, tie, xk, scale, maxD):
    """Which directed constructs the case holds, from the candidate sets (Frame.cc:549-587) of
    the final, shuffled right array."""
    out = {k: [] for k in ("best74", "best75", "best99", "tie_not_first", "at_minU", "at_maxU")}
    if len(kL) == 0 or len(kR) == 0:
        return out
    mnR, mxR = band(kR["y"], kR["octave"], scale)
    rowL = kL["y"].astype(np.int64)
    uL = kL["x"].astype(F)
    minU = (uL - F(maxD)).astype(F)
    cand = ((mnR[None, :] <= rowL[:, None]) & (mxR[None, :] >= rowL[:, None]) &
            (np.abs(kR["octave"][None, :].astype(np.int64) - kL["octave"][:, None]) <= 1) &
            (kR["x"][None, :] >= minU[:, None]) & (kR["x"][None, :] <= uL[:, None]))
    dist = np.full(cand.shape, 1000, np.int32)
    ci, cj = np.nonzero(cand)
    dist[ci, cj] = _POP[dL[ci] ^ dR[cj]].sum(axis=1)
    best = dist.min(axis=1)
    win = dist.argmin(axis=1)                       # the first (lowest iR) of equal distances
    bucket = kR["octave"].astype(np.int64) * 100000 + kR["y"].astype(np.int64)
    for i in np.nonzero(best < 100)[0]:
        w = win[i]
        if own[w] != i:
            continue
        if best[i] in (74, 75, 99):
            out[f"best{best[i]}"].append(int(i))
        if tie[w] >= 0:
            grp = np.nonzero((dist[i] == best[i]) & (tie == tie[w]) & (own == i))[0]
            if len(grp) >= 2 and bucket[w] > bucket[grp].min():
                out["tie_not_first"].append(int(i))
        if best[i] < 75 and xk[w] == 2 and kR["x"][w] == minU[i]:
            out["at_minU"].append(int(i))
        if best[i] < 75 and xk[w] == 0 and kR["x"][w] == uL[i]:
            out["at_maxU"].append(int(i))
    return out


def generate(base, seed, kind="regular", kp_cap=KP_CAP, mbf=MBF, mb=MB) -> Case:
    """The injected features of one pair over `base` (an entry of base_pairs())."""
    rng = np.random.default_rng(seed)
    maxD = float(F(F(mbf) / F(mb)))
    kL, dL, kR, dR, cons = _regular(base, rng, kp_cap, maxD)
    none = {k: [] for k in cons}
    ek, ed = np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8)
    if kind == "left_empty":
        kL, dL, cons = ek, ed, none
    elif kind == "right_empty":
        kR, dR, cons = ek, ed, none
    elif kind == "both_empty":
        kL, dL, kR, dR, cons = ek, ed, ek, ed, none
    elif kind == "one_each":
        # one left keypoint and one of its planted clones inside the band and the range
        i = int(rng.integers(0, len(kL)))
        kR, dR = kL[i:i + 1].copy(), dL[i:i + 1].copy()
        kR["x"] = F(kL["x"][i] - F(min(3.0, maxD / 2)))
        kL, dL, cons = kL[i:i + 1], dL[i:i + 1], none
    elif kind == "full_cap":
        # the left view filled to kp_cap with repeats of its keypoints
        rep = np.arange(kp_cap) % len(kL)
        kL, dL = kL[rep], dL[rep]
        cons = {k: np.nonzero(np.isin(rep, v))[0].tolist() for k, v in cons.items()}
    else:
        assert kind == "regular", kind
    assert len(kL) <= kp_cap and len(kR) <= kp_cap
    check_invariant(kL, kR, base["sizes"], base["scale"], base["inv_scale"])
    return Case(np.ascontiguousarray(kL), np.ascontiguousarray(dL), np.ascontiguousarray(kR),
                np.ascontiguousarray(dR), kind, base["index"], cons)


def batch_cases(bases, B):
    """The B cases of the regime test's batch of B pairs: pair p over base pair p % 4."""
    return [generate(bases[p % 4], pair_seed(B, p), pair_kind(B, p)) for p in range(B)]
