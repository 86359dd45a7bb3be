"""Directed cases for the ORBmatcher kernels (my_orb_slam2_amd/csrc/orbx_match.hip).

Every case is a small planted input (numpy only) that puts one of the reference's decisions
(src/ORBmatcher.cc) on its edge: descriptors at exact Hamming distances (a base descriptor
with a chosen number of bits flipped), keypoints at exact float32 coordinates, neighbouring
floats found with np.nextafter.  A case carries `probes`: (index, expected outcome, expected
match) for the features or queries it was planted for.  The expectations are written down
from the reference's rules and its float32 arithmetic, never taken from a matcher's output;
tests/test_oracle_match_directed.py checks them against the plain-Python restatement and the
oracle, tests/test_gpu_match_directed.py runs the same cases on the kernels.

Base descriptors are rows of the 256 x 256 Hadamard matrix: two different rows differ in
exactly 128 bits, so the groups of a case never come near each other's thresholds by chance.

Outcome codes (the restatements of tests/test_oracle_match.py produce the same strings):
  skipped          the feature / query is not processed (invalid, inactive, level > 0, ...)
  no_candidate     nothing left to compare with (empty window, everything filtered or claimed)
  over_threshold   the best distance fails the mode's threshold
  ratio_rejected   the best fails the ratio test against the second
  accepted         matched
  taken_over       (initialization) matched, then lost to a later query
  rotation_removed matched, then dropped by the rotation-consistency filter
A "+rescan" suffix: the decision was taken after the static best (or, where a second counts,
the static second) had been claimed by an earlier feature / query of the same call.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from my_orb_slam2_amd import synth
from my_orb_slam2_amd._lib import KEYPOINT_DTYPE
from my_orb_slam2_amd.features import (PROJ_FRAME_MAPPOINTS, PROJ_FUSE, PROJ_FUSE_SCW,
                                       PROJ_KEYFRAME, PROJ_KF_SCW, PROJ_LAST_FRAME,
                                       PROJ_QUERY_DTYPE, PROJ_SIM3, FeatureSet,
                                       assign_features_to_grid, feature_vector)

F = np.float32
WIDTH, HEIGHT = 752.0, 480.0
ORB_DIST = 64            # the ORBdist argument of every KEYFRAME case
FRAME_MODES = (PROJ_FRAME_MAPPOINTS, PROJ_LAST_FRAME, PROJ_KEYFRAME)
CLAIM_MODES = (PROJ_FRAME_MAPPOINTS, PROJ_KF_SCW, PROJ_LAST_FRAME, PROJ_KEYFRAME)
ALL_MODES = (PROJ_FRAME_MAPPOINTS, PROJ_KF_SCW, PROJ_LAST_FRAME, PROJ_KEYFRAME, PROJ_FUSE,
             PROJ_FUSE_SCW, PROJ_SIM3)
MODE_NAME = {PROJ_FRAME_MAPPOINTS: "frame_mappoints", PROJ_KF_SCW: "kf_scw",
             PROJ_LAST_FRAME: "last_frame", PROJ_KEYFRAME: "keyframe", PROJ_FUSE: "fuse",
             PROJ_FUSE_SCW: "fuse_scw", PROJ_SIM3: "sim3"}
MODE_TH = {PROJ_FRAME_MAPPOINTS: 100, PROJ_KF_SCW: 50, PROJ_LAST_FRAME: 100,
           PROJ_KEYFRAME: ORB_DIST, PROJ_FUSE: 50, PROJ_FUSE_SCW: 50, PROJ_SIM3: 100}

_H = (np.array([[bin(a & b).count("1") & 1 for b in range(256)] for a in range(256)], np.uint8))
HADAMARD = np.packbits(_H, axis=1)          # [256, 32]: rows pairwise at distance 128


def base(k: int) -> np.ndarray:
    return HADAMARD[k % 256].copy()


def flip(desc: np.ndarray, nbits: int, start: int = 0) -> np.ndarray:
    """`desc` with bits [start, start + nbits) flipped: at distance nbits from it."""
    d = desc.copy()
    for bit in range(start, start + nbits):
        d[bit // 8] ^= np.uint8(1 << (bit % 8))
    return d


def hd(a, b) -> int:
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def straddle(pred, lo, hi):
    """Adjacent float32 (t0, t1 = nextafter(t0, hi)) between lo and hi with
    pred(t0) == pred(lo) != pred(t1) == pred(hi): the two sides of a float comparison."""
    lo, hi = F(lo), F(hi)
    p_lo, p_hi = bool(pred(lo)), bool(pred(hi))
    assert p_lo != p_hi, "the predicate does not change between the ends"
    while True:
        nxt = np.nextafter(lo, hi)
        if nxt == hi:
            return lo, hi
        mid = F((np.float64(lo) + np.float64(hi)) / 2)
        if mid == lo or mid == hi:
            mid = nxt
        if bool(pred(mid)) == p_lo:
            lo = mid
        else:
            hi = mid


def ratio_accepts(d1: int, d2: int, ratio: float) -> bool:
    """static_cast<float>(bestDist1) < mfNNratio * static_cast<float>(bestDist2) (:262), in
    float32 as the reference evaluates it."""
    return bool(F(d1) < F(F(ratio) * F(d2)))


def float_double_disagreements(ratio: float, strict_less: bool, dmax: int = 100):
    """(d1, d2) pairs on which the float32 ratio test and the same test evaluated in double
    (with the float32 ratio) decide differently: d1 < r*d2 (strict_less) or d1 > r*d2."""
    out = []
    r = F(ratio)
    for d2 in range(1, 257):
        pf, pd = F(r * F(d2)), float(r) * d2
        for d1 in range(0, dmax + 1):
            a = (F(d1) < pf) if strict_less else (F(d1) > pf)
            b = (d1 < pd) if strict_less else (d1 > pd)
            if bool(a) != bool(b):
                out.append((d1, d2))
    return out


@dataclasses.dataclass
class Probe:
    index: int            # A / KF1 / F1 feature or query index
    expect: str           # outcome code
    match: int | None     # expected matched index (None = not stated)
    why: str = ""


class _Set:
    """Accumulates features; feature index = order of addition (also the order inside a
    FeatureVector node and a grid cell)."""

    def __init__(self):
        self.k, self.d, self.ur, self.node = [], [], [], []

    def add(self, desc, node=-1, x=400.0, y=240.0, octave=0, angle=0.0, ur=-1.0) -> int:
        self.k.append((F(x), F(y), F(31), F(angle), F(0), int(octave), -1))
        self.d.append(np.asarray(desc, np.uint8))
        self.ur.append(F(ur))
        self.node.append(int(node))
        return len(self.k) - 1

    def __len__(self):
        return len(self.k)

    def build(self) -> FeatureSet:
        keys = np.array(self.k, KEYPOINT_DTYPE) if self.k else np.zeros(0, KEYPOINT_DTYPE)
        desc = np.array(self.d, np.uint8).reshape(-1, 32)
        return FeatureSet(keys, desc, np.array(self.ur, F), feature_vector(np.array(self.node, np.int64)),
                          assign_features_to_grid(keys, 0.0, WIDTH, 0.0, HEIGHT))


# =============================================================================================
# SearchByBoW
# =============================================================================================

@dataclasses.dataclass
class BowCase:
    name: str
    a: FeatureSet
    va: np.ndarray
    b: FeatureSet
    vb: np.ndarray           # KF-KF only (all ones for KF-F)
    kf_kf: bool
    ratio: float
    check_ori: bool
    probes: list


class _Bow:
    def __init__(self, name, kf_kf, ratio, check_ori):
        self.name, self.kf_kf, self.ratio, self.check_ori = name, kf_kf, ratio, check_ori
        self.A, self.B, self.va, self.vb, self.probes = _Set(), _Set(), [], [], []
        self._node, self._row = 100, 0

    def node(self):
        self._node += 7
        return self._node

    def row(self):
        self._row += 1
        return base(self._row)

    def a(self, desc, node, valid=1, **kw):
        self.va.append(valid)
        return self.A.add(desc, node, **kw)

    def b(self, desc, node, valid=1, **kw):
        self.vb.append(valid)
        return self.B.add(desc, node, **kw)

    def probe(self, i, expect, match, why):
        self.probes.append(Probe(i, expect, match, why))

    def th_ok(self, d):
        return d < 50 if self.kf_kf else d <= 50

    def pair(self, d1, d2, why):
        """One A feature with a best at d1 and a second at d2 in a node of its own."""
        n, r = self.node(), self.row()
        i = self.a(r, n)
        j = self.b(flip(r, d1), n)
        self.b(flip(r, d2, 128), n)
        if not self.th_ok(d1):
            self.probe(i, "over_threshold", -1, why)
        elif not ratio_accepts(d1, d2, self.ratio):
            self.probe(i, "ratio_rejected", -1, why)
        else:
            self.probe(i, "accepted", j, why)
        return i

    def build(self) -> BowCase:
        return BowCase(self.name, self.A.build(), np.array(self.va, np.uint8), self.B.build(),
                       np.array(self.vb, np.uint8), self.kf_kf, self.ratio, self.check_ori,
                       self.probes)


def _bow_decisions(c: _Bow):
    """The threshold, ratio, tie, claim and node-set groups (no rotation filter)."""
    # A-only node below every shared id; B-only node below too: the first ids differ
    c.a(base(200), 3)
    c.b(base(201), 5)
    for d in (49, 50, 51):
        c.pair(d, 120, f"best {d}, far second")
    for d1, d2 in ((30, 50), (31, 50), (30, 49), (30, 40), (29, 40), (45, 50), (44, 50),
                   (9, 15), (8, 15)):
        c.pair(d1, d2, f"ratio {c.ratio}: {d1}/{d2}")
    # best and second at the same distance: the lower position is the best, second = best
    n, r = c.node(), c.row()
    i = c.a(r, n)
    c.b(flip(r, 20), n)
    c.b(flip(r, 20, 100), n)
    c.b(flip(r, 120, 128), n)
    c.probe(i, "ratio_rejected", -1, "best == second == 20")
    # ... and once the first of the two is claimed, the other is the best with a far second
    n, r = c.node(), c.row()
    t1 = flip(r, 20)
    i0 = c.a(t1, n)
    i1 = c.a(r, n)
    j1 = c.b(t1, n)
    j2 = c.b(flip(r, 20, 100), n)
    c.b(flip(r, 120, 128), n)
    c.probe(i0, "accepted", j1, "exact copy")
    c.probe(i1, "accepted+rescan", j2, "tie partner claimed: the other tied candidate wins")
    # every B feature of the node is claimed before the third A feature's turn
    n, r = c.node(), c.row()
    d0, d1 = r, flip(r, 100, 100)
    i0, i1, i2 = c.a(d0, n), c.a(d1, n), c.a(flip(r, 5), n)
    j0, j1 = c.b(d0, n), c.b(d1, n)
    c.probe(i0, "accepted", j0, "")
    c.probe(i1, "accepted+rescan", j1, "its static second is claimed")
    c.probe(i2, "no_candidate+rescan", -1, "the whole node is claimed")
    # a chain sharing one best: each later A feature is rescanned
    n, r = c.node(), c.row()
    ia = [c.a(r, n) for _ in range(4)]
    jb = [c.b(flip(r, d), n) for d in (0, 10, 30, 60)]
    c.b(flip(r, 120, 128), n)
    c.probe(ia[0], "accepted", jb[0], "chain 0/10")
    c.probe(ia[1], "accepted+rescan", jb[1], "chain 10/30")
    c.probe(ia[2], "accepted+rescan", jb[2], "chain 30/60")
    c.probe(ia[3], "over_threshold+rescan", -1, "chain 60")
    # the static SECOND is claimed and the rescan turns a ratio rejection into a match
    n, r = c.node(), c.row()
    y = flip(r, 25)
    i0, i1 = c.a(r, n), c.a(y, n)
    j0 = c.b(r, n)
    j1 = c.b(flip(y, 24, 100), n)
    c.b(flip(y, 120, 128), n)
    assert not ratio_accepts(24, 25, c.ratio) and ratio_accepts(24, 120, c.ratio)
    c.probe(i0, "accepted", j0, "")
    c.probe(i1, "accepted+rescan", j1, "static 24/25 rejects; second claimed: 24/120 accepts")
    # invalid A feature
    n, r = c.node(), c.row()
    i = c.a(r, n, valid=0)
    c.b(r, n)
    c.probe(i, "skipped", -1, "valid == 0")
    # KF-KF: the closest B feature has no MapPoint (ignored for KF-F, where it matches)
    n, r = c.node(), c.row()
    i = c.a(r, n)
    j0 = c.b(r, n, valid=0)
    j1 = c.b(flip(r, 10), n)
    c.b(flip(r, 120, 128), n)
    c.probe(i, "accepted", j1 if c.kf_kf else j0, "B feature without a MapPoint")
    # a shared node with a single feature on either side
    n, r = c.node(), c.row()
    i = c.a(r, n)
    j = c.b(flip(r, 7), n)
    c.probe(i, "accepted", j, "single candidate: second = 256")
    # ... whose only B feature has no MapPoint: KF-KF has nothing to compare with
    n, r = c.node(), c.row()
    i = c.a(r, n)
    j = c.b(r, n, valid=0)
    c.probe(i, "no_candidate" if c.kf_kf else "accepted", -1 if c.kf_kf else j,
            "the node's only B feature has no MapPoint")
    # ids A has and B lacks, and the reverse, between and after the shared ones
    i = c.a(c.row(), c.node())
    c.probe(i, "skipped", -1, "node id absent from B")
    c.b(c.row(), c.node())
    c.pair(10, 120, "shared node after unshared ones")
    c.b(base(202), 100000)
    c.a(base(203), 100001)
    return c


def _bow_node_sizes(c: _Bow, sizes):
    """Nodes of `sizes` A features: the first and the last one have an exact copy on the B
    side, the rest are 128 bits away from everything."""
    for s in sizes:
        n, r = c.node(), c.row()
        first, last, junk = flip(r, 3, 200), flip(r, 3, 210), c.row()
        ia = [c.a(first if k == 0 else last if k == s - 1 else junk, n) for k in range(s)]
        j_last = c.b(last, n)
        j_first = c.b(first, n)
        c.b(flip(r, 120, 60), n)
        j_far = len(c.B) - 1
        if s == 1:
            c.probe(ia[0], "accepted", j_first, "node of 1")
        else:
            c.probe(ia[0], "accepted", j_first, f"position 0 of {s}")
            c.probe(ia[-1], "accepted+rescan", j_last, f"position {s - 1} of {s}: its second is claimed")
            if s > 2:
                # junk: which two of the three B features are its static pair, by distance and position
                top2 = sorted((hd(junk, c.B.d[j]), j) for j in (j_last, j_first, j_far))[:2]
                c.probe(ia[s // 2], "over_threshold" + ("+rescan" if j_first in [j for _, j in top2] else ""),
                        -1, "junk")
    return c


# (count, A angle, B angle) groups of exact matches; `kept`: is the group's bin kept?
HISTOGRAMS = {
    "10_1": [(10, 0.0, 0.0, True), (1, 30.0, 0.0, True)],
    "20_2": [(20, 60.0, 0.0, True), (2, 0.0, 0.0, True)],
    "100_10_10": [(100, 0.0, 0.0, True), (10, 90.0, 0.0, True), (10, 30.0, 0.0, True)],
    "100_10_9": [(100, 0.0, 0.0, True), (10, 90.0, 0.0, True), (9, 30.0, 0.0, False)],
    "100_9": [(100, 0.0, 0.0, True), (9, 90.0, 0.0, False), (5, 30.0, 0.0, False)],
    "four_equal": [(4, 0.0, 0.0, True), (4, 30.0, 0.0, True), (4, 60.0, 0.0, True),
                   (4, 90.0, 0.0, False)],
    # 15 -> 0.5 -> bin 1; 45 -> bin 2 (1.5 rounds away); 345 -> bin 12; just below 360 -> bin 12;
    # a negative difference gets + 360 (10 - 350 -> 20 -> bin 1); 0 -> bin 0
    "angles": [(3, 15.0, 0.0, True), (2, 10.0, 350.0, True), (4, 45.0, 0.0, True),
               (2, 345.0, 0.0, True), (1, float(np.nextafter(F(360), F(0))), 0.0, True),
               (1, 0.0, 0.0, False), (1, 359.0, 359.5, True)],
}


def _bow_histogram(c: _Bow, groups):
    for cnt, a_ang, b_ang, kept in groups:
        for _ in range(cnt):
            n = c.node()     # a node per pair: no claim of another pair in sight
            r = c.row()
            i = c.a(r, n, angle=a_ang)
            j = c.b(r, n, angle=b_ang)
            c.probe(i, "accepted" if kept else "rotation_removed", j if kept else -1,
                    f"angles {a_ang} / {b_ang}")
    return c


def bow_cases() -> list:
    out = []
    for kf_kf in (False, True):
        fl = "kfkf" if kf_kf else "kff"
        for ratio in (0.6, 0.75, 0.9):
            out.append(_bow_decisions(_Bow(f"bow_{fl}_decisions_r{ratio}", kf_kf, ratio, False)).build())
        out.append(_bow_node_sizes(_Bow(f"bow_{fl}_nodes_small", kf_kf, 0.6, False),
                                   (1, 2, 63, 64, 65)).build())
        out.append(_bow_node_sizes(_Bow(f"bow_{fl}_nodes_1k", kf_kf, 0.6, False),
                                   (1023, 1024, 1025)).build())
        for name, groups in HISTOGRAMS.items():
            out.append(_bow_histogram(_Bow(f"bow_{fl}_hist_{name}", kf_kf, 0.6, True), groups).build())
    return out


def bow_regime_case(n: int, kf_kf: bool, single_node: bool, check_ori: bool = False,
                    seed: int = 5) -> BowCase:
    """n features per side (the size comes from orbx_matcher_variant): correlated random
    features in one node or in a many-node vocabulary, with the claim chain of
    `_bow_decisions` planted on the first features of one node."""
    f1, f2, _ = synth.feature_pair(seed, n1=n, n2=n, single_node=single_node)
    rng = np.random.default_rng(seed)
    va, vb = (rng.random(n) < 0.9).astype(np.uint8), (rng.random(n) < 0.9).astype(np.uint8)
    r = base(77)
    na = np.zeros(n, np.int64) if single_node else synth._node_of(f1.desc, 40)
    nb = np.zeros(n, np.int64) if single_node else synth._node_of(f2.desc, 40)
    node = int(na[0])
    for k, d in enumerate((0, 10, 30, 60)):
        f1.desc[k], f2.desc[k] = r, flip(r, d)
        na[k] = nb[k] = node
        va[k] = vb[k] = 1
    f2.desc[4] = flip(r, 120, 128)
    nb[4], vb[4] = node, 1
    f1.fvec, f2.fvec = feature_vector(na), feature_vector(nb)
    probes = [Probe(0, "accepted", 0, "chain"), Probe(1, "accepted+rescan", 1, "chain"),
              Probe(2, "accepted+rescan", 2, "chain"), Probe(3, "over_threshold+rescan", -1, "chain")]
    name = (f"bow_{'kfkf' if kf_kf else 'kff'}_{'one_node' if single_node else 'many_nodes'}_{n}"
            f"{'_ori' if check_ori else ''}")
    # what the rotation filter keeps of the planted chain depends on the random matches, so
    # with check_ori the case states no expectations
    return BowCase(name, f1, va, f2, vb if kf_kf else np.ones(n, np.uint8), kf_kf, 0.75,
                   check_ori, [] if check_ori else probes)


# =============================================================================================
# SearchForTriangulation
# =============================================================================================

@dataclasses.dataclass
class TriCase:
    name: str
    k1: FeatureSet
    h1: np.ndarray
    k2: FeatureSet
    h2: np.ndarray
    F12: np.ndarray
    epi: tuple
    only_stereo: bool
    check_ori: bool
    probes: list


# a = 0, b = 1, c = -y1: the epipolar line of kp1 is y = y1, num = y2 - y1, den = 1
F_ROWS = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], F)
# first two columns zero: a = b = 0, den == 0 for every kp1
F_DEN0 = np.array([0, 0, 1, 0, 0, 1, 0, 0, 1], F)
EPIPOLE = (F(300.0), F(50.0))
Y1 = F(200.0)


def chi2_ok(dy, octave=0) -> bool:
    """CheckDistEpipolarLine with F_ROWS for kp1.y = Y1, kp2.y = Y1 + dy (float32 steps, the
    last comparison in double)."""
    _, s2, _ = synth.scale_tables()
    y2 = F(Y1 + F(dy))
    c = F(F(F(0) + F(Y1 * F(-1))) + F(0))
    num = F(F(F(0) + F(F(1) * y2)) + c)
    dsqr = F(F(num * num) / F(1))
    return float(dsqr) < 3.84 * float(s2[octave])


def epipole_far(dx, octave=0) -> bool:
    """not (distex^2 + distey^2 < 100 * scale[octave]) for kp2 = (ex - dx, ey) (:791-798)."""
    s, _, _ = synth.scale_tables()
    x2 = F(EPIPOLE[0] - F(dx))
    distex = F(EPIPOLE[0] - x2)
    return not bool(F(F(distex * distex) + F(0)) < F(F(100) * s[octave]))


class _Tri:
    def __init__(self, name, only_stereo=False, check_ori=False, F12=F_ROWS):
        self.name, self.only_stereo, self.check_ori, self.F12 = name, only_stereo, check_ori, F12
        self.K1, self.K2, self.h1, self.h2, self.probes = _Set(), _Set(), [], [], []
        self._node, self._row = 50, 0

    node = _Bow.node
    row = _Bow.row
    probe = _Bow.probe

    def a(self, desc, node, has_mp=0, x=600.0, y=Y1, **kw):
        self.h1.append(has_mp)
        return self.K1.add(desc, node, x=x, y=y, **kw)

    def b(self, desc, node, has_mp=0, x=600.0, dy=0.0, y=None, **kw):
        self.h2.append(has_mp)
        return self.K2.add(desc, node, x=x, y=F(Y1 + F(dy)) if y is None else y, **kw)

    def build(self) -> TriCase:
        return TriCase(self.name, self.K1.build(), np.array(self.h1, np.uint8), self.K2.build(),
                       np.array(self.h2, np.uint8), self.F12.copy(), EPIPOLE, self.only_stereo,
                       self.check_ori, self.probes)


UR_VALUES = (("zero", 0.0), ("negzero", -0.0), ("minus1", -1.0), ("tiny", 1e-30))


def _tri_decisions(c: _Tri):
    mono_ok = not c.only_stereo     # a mono feature takes part at all
    ur = -1.0 if mono_ok else 5.0   # the plain groups: mono, or stereo under only_stereo

    def single(d, why, **kw):
        n, r = c.node(), c.row()
        i = c.a(r, n, ur=ur)
        j = c.b(flip(r, d), n, ur=ur, **kw)
        return i, j

    i, j = single(50, "50")
    c.probe(i, "accepted", j, "dist 50 passes")
    i, j = single(51, "51")
    c.probe(i, "no_candidate", -1, "dist 51 fails")
    # equal distances: the last accepted candidate in node order wins
    for cnt in (2, 3):
        n, r = c.node(), c.row()
        i = c.a(r, n, ur=ur)
        js = [c.b(flip(r, 30, 40 * k), n, ur=ur) for k in range(cnt)]
        c.probe(i, "accepted", js[-1], f"{cnt} candidates at 30: the last wins")
    n, r = c.node(), c.row()
    i = c.a(r, n, ur=ur)
    j0 = c.b(flip(r, 20), n, ur=ur)
    c.b(flip(r, 30, 100), n, ur=ur)
    c.probe(i, "accepted", j0, "a later, worse candidate does not displace")
    n, r = c.node(), c.row()
    i = c.a(r, n, ur=ur)
    c.b(flip(r, 30), n, ur=ur)
    j1 = c.b(flip(r, 20, 100), n, ur=ur)
    c.probe(i, "accepted", j1, "a later, better candidate displaces")
    # the last of three tied candidates fails the epipolar test: the second wins
    n, r = c.node(), c.row()
    i = c.a(r, n, ur=ur)
    c.b(flip(r, 30), n, ur=ur)
    j1 = c.b(flip(r, 30, 40), n, ur=ur)
    c.b(flip(r, 30, 80), n, ur=ur, dy=5.0)
    c.probe(i, "accepted", j1, "last tie off the epipolar line")
    # dsqr on either side of 3.84 * sigma2 (octaves 0 and 1)
    for o in (0, 1):
        lo, hi = straddle(lambda t: chi2_ok(t, o), 0.5, 4.0)
        assert chi2_ok(-lo, o) and not chi2_ok(-hi, o)
        for dy, ok in ((lo, True), (hi, False), (-lo, True), (-hi, False)):
            n, r = c.node(), c.row()
            i = c.a(r, n, ur=ur)
            j = c.b(flip(r, 5), n, ur=ur, dy=dy, octave=o)
            c.probe(i, "accepted" if ok else "no_candidate", j if ok else -1,
                    f"dsqr {'<' if ok else '>='} 3.84*sigma2[{o}] (dy {dy!r})")
    # KF1 feature already has a MapPoint; KF2 candidate has one
    n, r = c.node(), c.row()
    i = c.a(r, n, has_mp=1, ur=ur)
    c.b(r, n, ur=ur)
    c.probe(i, "skipped", -1, "KF1 feature has a MapPoint")
    n, r = c.node(), c.row()
    i = c.a(r, n, ur=ur)
    c.b(r, n, has_mp=1, ur=ur)
    j1 = c.b(flip(r, 9), n, ur=ur)
    c.probe(i, "accepted", j1, "closest KF2 candidate has a MapPoint")
    # the epipole cut, mono-mono only (octaves 0 and 1), and stereo features near the epipole
    for o in (0, 1):
        near, far = straddle(lambda t: epipole_far(t, o), 5.0, 15.0)
        for dx, ok in ((near, False), (far, True)):
            n, r = c.node(), c.row()
            i = c.a(r, n, y=EPIPOLE[1])
            j = c.b(r, n, x=F(EPIPOLE[0] - dx), y=EPIPOLE[1], octave=o)
            if not mono_ok:
                c.probe(i, "skipped", -1, "mono under only_stereo")
            else:
                c.probe(i, "accepted" if ok else "no_candidate", j if ok else -1,
                        f"epipole distance^2 {'>=' if ok else '<'} 100*scale[{o}]")
    for side in (1, 2):
        for nm, v in UR_VALUES:
            n, r = c.node(), c.row()
            i = c.a(r, n, y=EPIPOLE[1], ur=v if side == 1 else -1.0)
            j = c.b(r, n, x=EPIPOLE[0] - F(3), y=EPIPOLE[1], ur=v if side == 2 else -1.0)
            stereo = nm != "minus1"       # 0.0f, -0.0f and 1e-30 are all >= 0
            if c.only_stereo:
                c.probe(i, "skipped" if (side == 2 or not stereo) else "no_candidate", -1,
                        f"only_stereo, u_right {nm} on side {side}")
            else:
                c.probe(i, "accepted" if stereo else "no_candidate", j if stereo else -1,
                        f"3 px from the epipole, u_right {nm} on side {side}")
    return c


def _tri_node_sizes(c: _Tri, pairs=((63, 65), (64, 64), (65, 63), (129, 129), (1, 129))):
    """Nodes of sa KF1 and sb KF2 features: KF2 positions 0 and sb - 1 hold equal-distance
    copies for KF1's first and last feature (the last position wins across the 64-wide
    staging), everything else is 128 bits away."""
    for sa, sb in pairs:
        n, r = c.node(), c.row()
        junk = c.row()
        ia = [c.a(r if k in (0, sa - 1) else junk, n) for k in range(sa)]
        jb = [c.b(flip(r, 12, 20 * (k == 0)) if k in (0, sb - 1) else flip(junk, 90, 100), n)
              for k in range(sb)]
        c.probe(ia[0], "accepted", jb[-1], f"{sa} x {sb}: tie at positions 0 and {sb - 1}")
        c.probe(ia[-1], "accepted", jb[-1], f"{sa} x {sb}: last KF1 feature")
        if sa > 2:
            c.probe(ia[1], "no_candidate", -1, "junk")
    return c


def tri_cases() -> list:
    out = [_tri_decisions(_Tri("tri_decisions")).build(),
           _tri_decisions(_Tri("tri_decisions_only_stereo", only_stereo=True)).build(),
           _tri_node_sizes(_Tri("tri_node_sizes")).build()]
    c = _Tri("tri_den0", F12=F_DEN0)
    n, r = c.node(), c.row()
    i = c.a(r, n)
    c.b(r, n)
    c.probe(i, "no_candidate", -1, "den == 0")
    out.append(c.build())
    for name in ("10_1", "100_10_9", "four_equal", "angles"):
        c = _Tri(f"tri_hist_{name}", check_ori=True)
        n = c.node()
        for cnt, a_ang, b_ang, kept in HISTOGRAMS[name]:
            for _ in range(cnt):
                if len(c.K1) % 5 == 0:
                    n = c.node()
                r = c.row()
                i = c.a(r, n, angle=a_ang)
                j = c.b(r, n, angle=b_ang)
                c.probe(i, "accepted" if kept else "rotation_removed", j if kept else -1, "")
        out.append(c.build())
    return out


# =============================================================================================
# Projection searches
# =============================================================================================

@dataclasses.dataclass
class ProjCase:
    name: str
    mode: int
    target: FeatureSet
    q: np.ndarray
    qdesc: np.ndarray
    claimed: np.ndarray | None
    qflags: np.ndarray | None      # None: the plain entry point (and the batch form) apply
    prefilter: bool
    ratio: float
    check_ori: bool
    probes: list
    orb_dist: int = ORB_DIST


class _Proj:
    """Sites on a 30-pixel lattice (radius <= 8: the windows of two sites never meet)."""

    def __init__(self, name, mode, ratio=0.8, check_ori=False, ex=False, prefilter=False):
        self.name, self.mode, self.ratio, self.check_ori = name, mode, ratio, check_ori
        self.ex, self.prefilter = ex, prefilter
        self.T, self.claimed, self.q, self.qd, self.qf, self.probes = _Set(), [], [], [], [], []
        self._site, self._row = 0, 0
        self.frame = mode in FRAME_MODES

    row = _Bow.row
    probe = _Bow.probe

    def site(self):
        s = self._site
        self._site += 1
        assert s < 23 * 14
        return F(45.0 + 30.0 * (s % 23)), F(45.0 + 30.0 * (s // 23))

    def feat(self, desc, x, y, octave=0, angle=0.0, ur=-1.0, claimed=0):
        self.claimed.append(claimed)
        return self.T.add(desc, -1, x=x, y=y, octave=octave, angle=angle, ur=ur)

    def query(self, desc, u, v, radius=8.0, ur=0.0, levels=None, pred=0, angle=0.0, flag=0):
        if levels is None:
            levels = (-1, -1)
        self.q.append((F(u), F(v), F(ur), F(radius), levels[0], levels[1], pred, F(angle)))
        self.qd.append(np.asarray(desc, np.uint8))
        self.qf.append(flag)
        return len(self.q) - 1

    def pad_to(self, index):
        """Inactive and empty-window queries up to query position `index`."""
        while len(self.q) < index:
            k = len(self.q)
            self.query(base(250), 5.0, 470.0, radius=-1.0 if k % 2 else 3.0)

    def th(self):
        return MODE_TH[self.mode]

    def build(self) -> ProjCase:
        cl = np.array(self.claimed, np.uint8)
        return ProjCase(self.name, self.mode, self.T.build(), np.array(self.q, PROJ_QUERY_DTYPE),
                        np.array(self.qd, np.uint8).reshape(-1, 32),
                        cl if cl.any() else None,
                        np.array(self.qf, np.uint8) if self.ex else None, self.prefilter,
                        self.ratio, self.check_ori, self.probes)


def fuse_ok(u, x, stereo: bool) -> bool:
    """Fuse's chi-square cut (:968-992) for ex = u - x, ey = er = 0 at octave 0 (invSigma2 = 1)."""
    dx = F(F(u) - F(x))
    e2 = F(F(dx * dx) + F(0))
    if stereo:
        e2 = F(e2 + F(0))
    return not (float(F(e2 * F(1))) > (7.8 if stereo else 5.99))


WEIRD = [("u_nan", dict(u=np.nan)), ("v_nan", dict(v=np.nan)), ("u_pinf", dict(u=np.inf)),
         ("u_ninf", dict(u=-np.inf)), ("v_pinf", dict(v=np.inf)), ("v_ninf", dict(v=-np.inf)),
         ("u_1e12", dict(u=1e12)), ("u_m1e12", dict(u=-1e12)), ("v_1e12", dict(v=1e12)),
         ("v_m1e12", dict(v=-1e12)), ("r_zero", dict(radius=0.0)), ("r_neg", dict(radius=-2.0)),
         ("r_nan", dict(radius=np.nan)), ("r_inf", dict(radius=np.inf)),
         ("outside_left", dict(u=-40.0)), ("outside_right", dict(u=900.0)),
         ("outside_above", dict(v=-40.0)), ("outside_below", dict(v=600.0))]


def _proj_decisions(c: _Proj):
    """Window, level, threshold, stereo, chi-square and descriptor edges; every site has its
    own queries, so claims play no part here."""
    th = c.th()

    def one(d, why, fx=0.0, fy=0.0, expect=None, **qkw):
        u, v = c.site()
        r = c.row()
        j = c.feat(flip(r, d), F(u + F(fx)), F(v + F(fy)))
        i = c.query(r, u, v, **qkw)
        c.probe(i, expect or "accepted", j if (expect or "accepted") == "accepted" else -1, why)
        return i, j

    one(th, f"best == {th}")
    one(th + 1, f"best == {th + 1}", expect="over_threshold")
    # |dx| == r is outside (strict <), one float below is inside; the same for dy
    # (Fuse's chi-square cut is far inside a radius of 8: its windows here have radius 2)
    rr = 2.0 if c.mode == PROJ_FUSE else 8.0
    for sgn in (1.0, -1.0):
        u, v = c.site()
        edge = F(u + F(sgn * rr))
        inside = np.nextafter(edge, u)
        assert abs(F(edge - u)) == F(rr) and abs(F(inside - u)) < F(rr)
        r = c.row()
        c.feat(r, edge, v)
        c.probe(c.query(r, u, v, radius=rr), "no_candidate", -1, f"dx == {sgn * rr}")
        u, v = c.site()
        r = c.row()
        j = c.feat(r, np.nextafter(F(u + F(sgn * rr)), u), v)
        c.probe(c.query(r, u, v, radius=rr), "accepted", j, "|dx| one float below r")
        u, v = c.site()
        r = c.row()
        c.feat(r, u, F(v + F(sgn * rr)))
        c.probe(c.query(r, u, v, radius=rr), "no_candidate", -1, f"dy == {sgn * rr}")
        u, v = c.site()
        r = c.row()
        j = c.feat(r, u, np.nextafter(F(v + F(sgn * rr)), v))
        c.probe(c.query(r, u, v, radius=rr), "accepted", j, "|dy| one float below r")
    # windows that start left of / above the grid and end right of / below it
    for x, y, u, v in ((1.0, 200.0, 3.0, 200.0), (300.0, 1.0, 300.0, 3.0),
                       (745.0, 300.0, 747.0, 300.0), (400.0, 474.0, 400.0, 476.0),
                       (1.0, 1.0, 0.0, -1.0)):
        r = c.row()
        j = c.feat(r, x, y)
        c.probe(c.query(r, u, v), "accepted", j, f"window over the grid edge at ({u}, {v})")
    # non-finite, huge and outside queries
    u0, v0 = c.site()
    r0 = c.row()
    c.feat(r0, u0, v0)
    for nm, kw in WEIRD:
        a = dict(u=u0, v=v0, radius=8.0)
        a.update(kw)
        i = c.query(r0, a["u"], a["v"], radius=a["radius"])
        c.probe(i, "skipped" if nm in ("r_neg", "r_nan") else "no_candidate", -1, nm)
    # a radius of 3e9 covers the whole grid: the exact copy wins over every other feature
    c.probe(c.query(r0, u0, v0, radius=3e9), "accepted", len(c.T) - 1, "radius 3e9")
    # a descriptor and its complement
    one(0, "distance 256", expect="no_candidate" if c.mode in (
        PROJ_FRAME_MAPPOINTS, PROJ_KF_SCW, PROJ_LAST_FRAME, PROJ_KEYFRAME, PROJ_FUSE)
        else "over_threshold")
    c.T.d[-1] = np.bitwise_not(c.T.d[-1])
    # levels: candidates at octaves 0 / 1 / 7 at distances 10 / 20 / 30
    if c.frame:
        for lv2, want in (((-1, -1), 0), ((0, -1), 0), ((1, -1), 1), ((0, 0), 0), ((0, 1), 0),
                          ((6, 7), 7), ((7, 7), 7), ((2, 5), None), ((8, -1), None)):
            u, v = c.site()
            r = c.row()
            js = {o: c.feat(flip(r, d), F(u + F(k)), v, octave=o)
                  for k, (o, d) in enumerate(((0, 10), (1, 20), (7, 30)))}
            i = c.query(r, u, v, levels=lv2)
            c.probe(i, "accepted" if want is not None else "no_candidate",
                    js[want] if want is not None else -1, f"levels {lv2}")
    else:
        for pred, want in ((0, 0), (1, 0), (2, 1), (7, 7), (8, 7), (9, None), (4, None)):
            u, v = c.site()
            r = c.row()
            js = {o: c.feat(flip(r, d), F(u + F(k)), v, octave=o)
                  for k, (o, d) in enumerate(((0, 10), (1, 20), (7, 30)))}
            i = c.query(r, u, v, pred=pred)
            c.probe(i, "accepted" if want is not None else "no_candidate",
                    js[want] if want is not None else -1, f"pred_level {pred}")
    # the stereo check of the frame projections: uRight > 0 only
    if c.mode in (PROJ_FRAME_MAPPOINTS, PROJ_LAST_FRAME):
        for ur_f, ur_q, ok, why in ((50.0, 58.0, True, "|ur - uRight| == r"),
                                    (50.0, float(np.nextafter(F(58), F(60))), False, "one float above r"),
                                    (0.0, 1000.0, True, "uRight == 0.0f: no stereo check"),
                                    (-0.0, 1000.0, True, "uRight == -0.0f"),
                                    (1e-30, 1000.0, False, "tiny positive uRight"),
                                    (-1.0, 1000.0, True, "monocular")):
            u, v = c.site()
            r = c.row()
            j = c.feat(r, u, v, ur=ur_f)
            c.probe(c.query(r, u, v, ur=ur_q), "accepted" if ok else "no_candidate",
                    j if ok else -1, why)
    if c.mode == PROJ_FUSE:
        for stereo in (False, True):
            for k in range(2):
                u, v = c.site()
                lo, hi = straddle(lambda x: fuse_ok(u, x, stereo), u - F(1), u - F(4))
                x, ok = (lo, True) if k == 0 else (hi, False)
                r = c.row()
                j = c.feat(r, x, v, ur=30.0 if stereo else -1.0)
                c.probe(c.query(r, u, v, ur=30.0), "accepted" if ok else "no_candidate",
                        j if ok else -1, f"chi2 {'stereo' if stereo else 'mono'} x {x!r}")
        # e2 = 6.5: inside the stereo cut (7.8), outside the mono cut (5.99)
        dx = F(2.5)
        assert not fuse_ok(dx, 0.0, False) and fuse_ok(dx, 0.0, True)
        for ur_f, ok in ((0.0, True), (-0.0, True), (-1.0, False)):
            u, v = c.site()
            r = c.row()
            j = c.feat(r, F(u - dx), v, ur=ur_f)
            c.probe(c.query(r, u, v, ur=0.0), "accepted" if ok else "no_candidate",
                    j if ok else -1, f"u_right {ur_f!r}: {'stereo' if ok else 'mono'} branch")
    if c.mode == PROJ_FRAME_MAPPOINTS:
        pairs = [(40, 50), (41, 50), (45, 50), (46, 50), (80, 100), (81, 100)]
        pairs += [p for p in float_double_disagreements(c.ratio, False) if p[1] <= 120][:2]
        for d1, d2 in pairs:
            rej = bool(F(d1) > F(F(c.ratio) * F(d2)))
            for same in (True, False):
                u, v = c.site()
                r = c.row()
                j = c.feat(flip(r, d1), u, v, octave=2)
                c.feat(flip(r, d2, 128), F(u + F(1)), v, octave=2 if same else 3)
                i = c.query(r, u, v, levels=(2, 3))
                bad = rej and same
                c.probe(i, "ratio_rejected" if bad else "accepted", -1 if bad else j,
                        f"{d1}/{d2} ratio {c.ratio} {'same' if same else 'other'} level")
        one(100, "single candidate: second = 256 at level -1")
    return c


def _proj_claims(c: _Proj):
    """The replay's structure: shared features, candidate lists of 8 and of 9 or more with
    their heads claimed, at chosen lanes of the 64-query chunks.  129 queries."""
    assert c.mode in CLAIM_MODES

    def ladder(nfeat, pre=()):
        """A site of nfeat features at distances 1..nfeat from its base descriptor."""
        u, v = c.site()
        r = c.row()
        # neighbours in distance sit at different levels (2, 3, 2, ...): FRAME_MAPPOINTS' ratio
        # test applies to equal levels only, so it never decides here
        js = [c.feat(flip(r, k + 1), F(u + F(k % 3 - 1)), F(v + F(k // 3 - 1)), octave=2 + k % 2,
                     claimed=int(k in pre)) for k in range(nfeat)]
        return u, v, r, js

    def claimers(s, ks):
        u, v, r, js = s
        for k in ks:   # the k-th feature's own descriptor: distance 0 to it
            i = c.query(flip(r, k + 1), u, v, levels=(2, 3) if c.frame else None, pred=3)
            c.probe(i, "accepted", js[k], f"claims ladder step {k}")

    def final(s, want, why, flag=0):
        u, v, r, js = s
        i = c.query(r, u, v, levels=(2, 3) if c.frame else None, pred=3, flag=flag)
        c.probe(i, "accepted+rescan", js[want], why)
        return i

    s1, s2, s3, s4, s5, s6 = ladder(9), ladder(9), ladder(8), ladder(10), ladder(12), ladder(9)
    claimers(s1, range(8))                                   # 0..7
    final(s1, 8, "list of 9, first 8 taken (chunk 0, lane 8)")
    for s, cnt in ((s2, 7), (s3, 7), (s4, 8), (s5, 8), (s6, 8)):
        claimers(s, range(cnt))                              # 9..46
    # a feature claimed before the call is out of every list: the next one is the best
    s7 = ladder(4, pre=(0,))
    i = c.query(s7[2], s7[0], s7[1], levels=(2, 3) if c.frame else None, pred=3)
    c.probe(i, "accepted", s7[3][1], "closest feature claimed before the call")
    # two, three and nine queries wanting one feature (nothing else in the window)
    for cnt in (2, 3, 9):
        u, v = c.site()
        r = c.row()
        j = c.feat(flip(r, 2), u, v, octave=2)
        for k in range(cnt):
            i = c.query(r, u, v, levels=(2, 3) if c.frame else None, pred=3)
            c.probe(i, "accepted" if k == 0 else "no_candidate+rescan", j if k == 0 else -1,
                    f"query {k} of {cnt} wanting one feature")
    assert len(c.q) <= 63
    c.pad_to(63)
    final(s2, 7, "list of 9, first 7 taken (chunk 0, lane 63)")
    final(s4, 8, "list of 10, first 8 taken (chunk 1, lane 0)")
    final(s5, 8, "list of 12, first 8 taken (chunk 1, lane 1)")
    final(s3, 7, "list of exactly 8, first 7 taken: decided from the list")
    c.pad_to(127)
    final(s6, 8, "list of 9, first 8 taken (chunk 1, lane 63)")
    u, v, r, js = s1
    i = c.query(r, u, v, levels=(2, 3) if c.frame else None, pred=3)
    c.probe(i, "no_candidate+rescan", -1, "every feature of the site is claimed (chunk 2)")
    assert len(c.q) == 129
    return c


def _proj_no_claim(c: _Proj):
    """ORBX_QF_NO_CLAIM queries before and after a claiming query for the same feature."""
    reads = c.mode in (PROJ_FRAME_MAPPOINTS, PROJ_LAST_FRAME)
    for order in ("before", "after", "two_before"):
        u, v = c.site()
        r = c.row()
        j = c.feat(flip(r, 3), u, v)
        flags = {"before": (1, 0, 0), "after": (0, 1, 1), "two_before": (1, 1, 0, 0)}[order]
        taken = False
        for k, fl in enumerate(flags):
            i = c.query(r, u, v, flag=fl)
            c.probe(i, ("no_candidate+rescan" if taken else "accepted"), -1 if taken else j,
                    f"{order}: query {k} flag {fl}")
            if not (fl and reads):
                taken = True
    # a no-claim query in the last lane of chunk 0, the claiming one first in chunk 1
    c.pad_to(63)
    u, v = c.site()
    r = c.row()
    j = c.feat(flip(r, 3), u, v)
    i0, i1 = c.query(r, u, v, flag=1), c.query(r, u, v, flag=0)
    c.probe(i0, "accepted", j, "no-claim, lane 63")
    c.probe(i1, "accepted" if reads else "no_candidate+rescan", j if reads else -1,
            "claiming query, next chunk")
    return c


def _proj_histogram(c: _Proj, groups):
    for cnt, a_ang, b_ang, kept in groups:
        for _ in range(cnt):
            u, v = c.site()
            r = c.row()
            j = c.feat(r, u, v, angle=b_ang)
            i = c.query(r, u, v, angle=a_ang)
            c.probe(i, "accepted" if kept else "rotation_removed", j if kept else -1, "")
    return c


def proj_cases() -> list:
    out = []
    for mode in ALL_MODES:
        nm = MODE_NAME[mode]
        out.append(_proj_decisions(_Proj(f"proj_{nm}_decisions", mode)).build())
        if mode in CLAIM_MODES:
            out.append(_proj_claims(_Proj(f"proj_{nm}_claims", mode)).build())
            out.append(_proj_claims(_Proj(f"proj_{nm}_claims_ex", mode, ex=True)).build())
            out.append(_proj_no_claim(_Proj(f"proj_{nm}_no_claim", mode, ex=True)).build())
    out.append(_proj_decisions(_Proj("proj_frame_mappoints_decisions_r0.9", PROJ_FRAME_MAPPOINTS,
                                     ratio=0.9)).build())
    for mode in (PROJ_FRAME_MAPPOINTS, PROJ_LAST_FRAME):
        out.append(_proj_no_claim(_Proj(f"proj_{MODE_NAME[mode]}_no_claim_prefilter", mode, ex=True,
                                        check_ori=True, prefilter=True)).build())
    for mode in (PROJ_LAST_FRAME, PROJ_KEYFRAME):
        for name in ("10_1", "20_2", "100_10_10", "100_10_9", "100_9", "four_equal", "angles"):
            out.append(_proj_histogram(_Proj(f"proj_{MODE_NAME[mode]}_hist_{name}", mode,
                                             check_ori=True), HISTOGRAMS[name]).build())
        out.append(_proj_histogram(_Proj(f"proj_{MODE_NAME[mode]}_hist_100_9_prefilter", mode,
                                         check_ori=True, ex=True, prefilter=True),
                                   [(c, a, b, True) for c, a, b, _ in HISTOGRAMS["100_9"]]).build())
    # query counts around the 64-query chunk: the first nq queries of the claims case
    for mode in CLAIM_MODES:
        for nq in (63, 64, 65):
            c = _proj_claims(_Proj(f"proj_{MODE_NAME[mode]}_claims_nq{nq}", mode))
            c.q, c.qd, c.qf = c.q[:nq], c.qd[:nq], c.qf[:nq]
            c.probes = [p for p in c.probes if p.index < nq]
            out.append(c.build())
    return out


def proj_regime_case(n_target: int, mode: int, ex: bool, nq: int = 2000, seed: int = 9) -> ProjCase:
    """A target of n_target features (the size comes from orbx_matcher_variant) with about nq
    queries: random correlated features, dense windows (truncated lists), and on top the nine
    queries wanting one feature and a list of 9 with its first 8 taken, planted in a corner
    that the random features are kept out of."""
    n1 = nq - 20
    f1, f2, t = synth.feature_pair(seed, n1=n1, n2=n_target - 10, dup_frac=0.1)
    keep = ~((f2.keys["x"] < 40) & (f2.keys["y"] < 40))
    f2.keys["x"][~keep] += 60
    q, d = synth.projection_queries(seed, f1, f2, t, th=6.0,
                                    mode_levels="frame" if mode in FRAME_MODES else "kf")
    q["u"][(q["u"] < 50) & (q["v"] < 50)] += 70
    keys = np.zeros(10, KEYPOINT_DTYPE)
    r = base(9)
    keys["x"], keys["y"], keys["octave"] = 10.0, 10.0, 2
    keys["x"][:9] += np.arange(9) % 3 - 1
    keys["x"][9], keys["y"][9] = 25.0, 25.0
    pd = np.array([flip(r, k + 1) for k in range(9)] + [flip(base(10), 2)], np.uint8)
    n0 = f2.n
    T = FeatureSet(np.concatenate([f2.keys, keys]), np.concatenate([f2.desc, pd]),
                   np.concatenate([f2.u_right, np.full(10, -1, F)]), None, None)
    T.grid = assign_features_to_grid(T.keys, 0.0, WIDTH, 0.0, HEIGHT)
    pq = np.zeros(19, PROJ_QUERY_DTYPE)
    pq["u"], pq["v"], pq["radius"], pq["pred_level"] = 10.0, 10.0, 4.0, 2
    pq["min_level"], pq["max_level"] = ((2, 2) if mode in FRAME_MODES else (-1, -1))
    pq["u"][9:], pq["v"][9:], pq["radius"][9:] = 25.0, 25.0, 2.0
    pqd = np.array([flip(r, k + 1) for k in range(8)] + [r] + [base(10)] * 10, np.uint8)
    at = 600                       # plant the block across a chunk boundary region
    Q = np.concatenate([q[:at], pq, q[at:]])
    D = np.concatenate([d[:at], pqd, d[at:]])
    probes = [Probe(at + k, "accepted", n0 + k, "ladder claimer") for k in range(8)]
    probes.append(Probe(at + 8, "accepted+rescan", n0 + 8, "list of 9, first 8 taken"))
    probes += [Probe(at + 9 + k, "accepted" if k == 0 else "no_candidate+rescan",
                     n0 + 9 if k == 0 else -1, "ten want one") for k in range(10)]
    rng = np.random.default_rng(seed)
    claimed = (rng.random(T.n) < 0.1).astype(np.uint8)
    claimed[n0:] = 0
    qflags = None
    if ex:
        qflags = (rng.random(len(Q)) < 0.3).astype(np.uint8)
        qflags[at:at + 19] = 0
    return ProjCase(f"proj_{MODE_NAME[mode]}_target_{n_target}{'_ex' if ex else ''}", mode, T, Q, D,
                    claimed, qflags, ex and mode != PROJ_FRAME_MAPPOINTS, 0.8, True, probes)


# =============================================================================================
# SearchForInitialization
# =============================================================================================

@dataclasses.dataclass
class InitCase:
    name: str
    f1: FeatureSet
    f2: FeatureSet
    prev: np.ndarray          # [n1, 2] float32 (vbPrevMatched); copy before use
    window: int
    ratio: float
    check_ori: bool
    probes: list


def init_cases() -> list:
    out = []
    for ratio in (0.9, 0.6):
        c = _Proj(f"init_decisions_r{ratio}", -1, ratio=ratio)
        A, prev = _Set(), []

        def f1(desc, u, v, octave=0, angle=0.0, _A=A, _prev=prev):
            _prev.append((F(u + F(1)), F(v - F(1))))     # vbPrevMatched, not the keypoint
            return _A.add(desc, -1, x=u, y=v, octave=octave, angle=angle)

        def pair(d1, d2, why):
            u, v = c.site()
            r = c.row()
            j = c.feat(flip(r, d1), u, v)
            if d2 is not None:
                c.feat(flip(r, d2, 128), F(u + F(2)), v)
            i = f1(r, u, v)
            if d1 > 50:
                c.probe(i, "over_threshold", -1, why)
            elif d2 is not None and not bool(F(d1) < F(F(d2) * F(ratio))):
                c.probe(i, "ratio_rejected", -1, why)
            else:
                c.probe(i, "accepted", j, why)

        pair(50, None, "50, no second")
        pair(51, None, "51")
        for d1, d2 in ((30, 50), (31, 50), (45, 50), (44, 50), (30, 40), (29, 40), (9, 15)):
            pair(d1, d2, f"ratio {ratio}: {d1}/{d2}")
        # level-1 feature: inactive
        u, v = c.site()
        r = c.row()
        c.feat(r, u, v)
        c.probe(f1(r, u, v, octave=1), "skipped", -1, "level 1")
        # F2 candidate at octave 1: outside (level1, level1) = (0, 0)
        u, v = c.site()
        r = c.row()
        c.feat(r, u, v, octave=1)
        c.probe(f1(r, u, v), "no_candidate", -1, "F2 feature at level 1")
        # take-overs: a later query with a strictly smaller distance wins the feature
        u, v = c.site()
        r = c.row()
        j = c.feat(r, u, v)
        i0, i1 = f1(flip(r, 20), u, v), f1(flip(r, 10), u, v)
        c.probe(i0, "taken_over", -1, "20, then 10 arrives")
        c.probe(i1, "accepted", j, "10 takes the feature")
        u, v = c.site()
        r = c.row()
        j = c.feat(r, u, v)
        i0, i1 = f1(flip(r, 20), u, v), f1(flip(r, 20, 100), u, v)
        c.probe(i0, "accepted", j, "first at 20 keeps the feature")
        c.probe(i1, "no_candidate+rescan", -1, "equal distance: vMatchedDistance <= dist skips")
        u, v = c.site()
        r = c.row()
        j = c.feat(r, u, v)
        ii = [f1(flip(r, d), u, v) for d in (30, 20, 10, 10)]
        for i in ii[:2]:
            c.probe(i, "taken_over", -1, "chain of take-overs")
        c.probe(ii[2], "accepted", j, "end of the chain")
        c.probe(ii[3], "no_candidate+rescan", -1, "equal to the holder")
        # a later query prefers a held feature it cannot take and falls back to its second
        u, v = c.site()
        r = c.row()
        j0 = c.feat(r, u, v)
        j1 = c.feat(flip(r, 40, 128), F(u + F(2)), v)
        i0, i1 = f1(r, u, v), f1(flip(r, 5), u, v)
        c.probe(i0, "accepted", j0, "")
        c.probe(i1, "accepted+rescan", j1,
                "best held at a smaller distance: the other candidate wins")
        case = c.build()
        out.append(InitCase(c.name, A.build(), case.target, np.array(prev, F).reshape(-1, 2), 8,
                            ratio, False, c.probes))
    for name in ("10_1", "100_10_9", "four_equal"):
        c = _Proj(f"init_hist_{name}", -1, ratio=0.9)
        A, prev = _Set(), []
        for cnt, a_ang, b_ang, kept in HISTOGRAMS[name]:
            for _ in range(cnt):
                u, v = c.site()
                r = c.row()
                j = c.feat(r, u, v, angle=b_ang)
                i = A.add(r, -1, x=u, y=v, angle=a_ang)
                prev.append((F(u - F(2)), F(v + F(1))))
                c.probe(i, "accepted" if kept else "rotation_removed", j if kept else -1, "")
        out.append(InitCase(c.name, A.build(), c.build().target, np.array(prev, F).reshape(-1, 2),
                            8, 0.9, True, c.probes))
    return out


# =============================================================================================
# MapPoint::ComputeDistinctiveDescriptors
# =============================================================================================

def distinctive_case():
    """(desc, off, expect): point p's rows are desc[off[p]:off[p + 1]]."""
    rows, off, expect = [], [0], []

    def point(ds, want):
        rows.extend(ds)
        off.append(len(rows))
        expect.append(want)

    r = base(1)
    point([], -1)                                             # N = 0
    point([r], 0)                                             # N = 1
    point([r, flip(r, 9)], 0)                                 # N = 2: medians 0, 0 -> first
    # N = 3: medians 10, 3, 3: rows 1 and 2 tie, the first wins
    point([flip(r, 10, 100), r, flip(r, 3)], 1)
    # N = 4: index (N-1)/2 = 1 of the sorted row (the second smallest)
    point([flip(r, 20), r, flip(r, 2), flip(r, 30, 100)], 1)
    point([r] * 5, 0)                                         # all equal
    # two rows tie for the least median: identical rows 2 and 4 among spread ones
    point([flip(r, 60), flip(r, 60, 100), r, flip(r, 50, 180), r, flip(r, 1)], 2)
    rng = np.random.default_rng(3)
    for n in (63, 64, 65, 256):
        # row `want` is the base; the others are the base with 20..60 random bits flipped
        want = n - 1 if n != 64 else 0
        ds = []
        for k in range(n):
            d = r.copy()
            if k != want:
                bits = rng.choice(256, size=int(rng.integers(20, 61)), replace=False)
                np.bitwise_xor.at(d, bits // 8, (1 << (bits % 8)).astype(np.uint8))
            ds.append(d)
        point(ds, want)
    return (np.array(rows, np.uint8).reshape(-1, 32), np.array(off, np.int32),
            np.array(expect, np.int32))


# =============================================================================================
# Size regimes
# =============================================================================================

def scan_regimes(variant, kind: int, nq: int = 0, limit: int = 40000) -> dict:
    """Scans orbx_matcher_variant (`variant(kind, n_a, n_b, nq)`) over equal-sided sizes n = 1,
    2, ... and returns the sizes at which its answer changes: "last_on_chip" (the largest n
    answering 0 before the first other answer), "first_fallback" (the smallest n answering 1,
    or None), "first_error" (the smallest n with a negative answer) and "error" (that answer).
    """
    out = dict(last_on_chip=None, first_fallback=None, first_error=None, error=None)
    for n in range(1, limit):
        v = variant(kind, n, n, nq)
        if v == 0 and out["first_fallback"] is None:
            out["last_on_chip"] = n
        elif v == 1 and out["first_fallback"] is None:
            out["first_fallback"] = n
        elif v < 0:
            out["first_error"], out["error"] = n, v
            break
    return out
