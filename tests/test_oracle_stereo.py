"""Frame::ComputeStereoMatches of the oracle against an independent Python reading, and the
coverage of the directed stereo cases (tests/stereo_cases.py).

The GPU stereo tests compare k_stereo with oracle_stereo_match alone, so the oracle's matcher
gets its own check here: `reference_stereo` is written from the reference's text
(src/Frame.cc:496-686), one statement at a time, in numpy float32 where the reference has
`float`, and is compared with oracle_stereo_match_ex bit for bit (uRight, depth), in the valid
count and in the exit every left keypoint took, on plain extracted pairs and on injected ones.
The second half runs the oracle over the exact case sets of tests/test_gpu_stereo_directed.py
and asserts that every exit and every directed construct is present in every batch: what the
GPU test proves is what these floors say it ran.
"""
import numpy as np
import pytest

import stereo_cases as sc

F = np.float32
TH_HIGH, TH_LOW = 100, 50            # ORBmatcher::TH_HIGH / TH_LOW (src/ORBmatcher.cc:37-38)
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def _round(x):
    """std::round on a float: half away from zero."""
    x = F(x)
    return F(np.copysign(np.floor(np.abs(x) + F(0.5)), x))


def reference_stereo(kL, dL, kR, dR, levelsL, levelsR, scale, inv_scale, mbf, mb):
    """src/Frame.cc:496-686.  levelsL / levelsR: mvImagePyramid of the two extractors (uint8
    arrays).  Returns (mvuRight, mvDepth, valid count, exit code per left keypoint); the codes
    are those of oracle_stereo_match_ex (oracle/orb_oracle.h)."""
    N = len(kL)
    mvuRight = np.full(N, -1.0, F)                                  # :498-499
    mvDepth = np.full(N, -1.0, F)
    why = np.full(N, -1, np.int32)
    thOrbDist = (TH_HIGH + TH_LOW) // 2                             # :501
    nRows = levelsL[0].shape[0]                                     # :503
    vRowIndices = [[] for _ in range(nRows)]                        # :511
    for iR in range(len(kR)):                                       # :518-531
        kpY = F(kR["y"][iR])
        r = F(F(2.0) * F(scale[kR["octave"][iR]]))
        maxr = int(np.ceil(F(kpY + r)))
        minr = int(np.floor(F(kpY - r)))
        for yi in range(minr, maxr + 1):
            assert 0 <= yi < nRows, "right keypoint band outside the image (undefined in the reference)"
            vRowIndices[yi].append(iR)
    minZ = F(mb)                                                    # :534-536
    minD = F(0)
    maxD = F(F(mbf) / minZ)
    vDistIdx = []
    for iL in range(N):                                             # :542
        levelL = int(kL["octave"][iL])
        vL, uL = F(kL["y"][iL]), F(kL["x"][iL])
        vCandidates = vRowIndices[int(vL)]                          # :549 (float -> size_t)
        why[iL] = 2
        if not vCandidates:
            continue
        minU = F(uL - maxD)                                         # :554-555
        maxU = F(uL - minD)
        if maxU < 0:
            continue
        bestDist = TH_HIGH                                          # :560-561
        bestIdxR = 0
        for iR in vCandidates:                                      # :566-587
            octR = int(kR["octave"][iR])
            if octR < levelL - 1 or octR > levelL + 1:
                continue
            uR = F(kR["x"][iR])
            if uR >= minU and uR <= maxU:
                dist = int(_POP[dL[iL] ^ dR[iR]].sum())
                if dist < bestDist:
                    bestDist = dist
                    bestIdxR = iR
        why[iL] = 3 if bestDist >= TH_HIGH else 4
        if not bestDist < thOrbDist:                                # :591
            continue
        uR0 = F(kR["x"][bestIdxR])                                  # :594-598
        scaleFactor = F(inv_scale[levelL])
        scaleduL = _round(uL * scaleFactor)
        scaledvL = _round(vL * scaleFactor)
        scaleduR0 = _round(uR0 * scaleFactor)
        w = 5                                                       # :601-604
        PL, PR = levelsL[levelL], levelsR[levelL]
        y0, x0 = int(scaledvL - F(w)), int(scaleduL - F(w))
        assert y0 >= 0 and x0 >= 0 and y0 + 11 <= PL.shape[0] and x0 + 11 <= PL.shape[1]
        IL = PL[y0:y0 + 2 * w + 1, x0:x0 + 2 * w + 1].astype(F)
        IL = IL - IL[w, w]
        bestDistS = 2 ** 31 - 1                                     # :606-610
        bestincR = 0
        L = 5
        vDists = np.zeros(2 * L + 1, F)
        iniu = F(scaleduR0 + F(L) - F(w))                           # :612-615
        endu = F(scaleduR0 + F(L) + F(w) + F(1))
        why[iL] = 9
        if iniu < 0 or endu >= PR.shape[1]:
            continue
        for incR in range(-L, L + 1):                               # :617-631
            xr = int(F(scaleduR0 + F(incR) - F(w)))
            assert xr >= 0 and xr + 11 <= PR.shape[1]
            IR = PR[y0:y0 + 2 * w + 1, xr:xr + 2 * w + 1].astype(F)
            IR = IR - IR[w, w]
            dist = F(np.abs(IL.astype(np.float64) - IR.astype(np.float64)).sum())   # cv::norm L1
            if dist < F(bestDistS):
                bestDistS = int(dist)
                bestincR = incR
            vDists[L + incR] = dist
        why[iL] = 5
        if bestincR == -L or bestincR == L:                         # :633
            continue
        dist1, dist2, dist3 = vDists[L + bestincR - 1], vDists[L + bestincR], vDists[L + bestincR + 1]
        with np.errstate(divide="ignore", invalid="ignore"):        # :644
            deltaR = F(F(dist1 - dist3) / F(F(2.0) * F(F(dist1 + dist3) - F(F(2.0) * dist2))))
        why[iL] = 6
        if deltaR < -1 or deltaR > 1:                               # :646
            continue
        bestuR = F(F(scale[levelL]) * F(F(scaleduR0 + F(bestincR)) + deltaR))   # :653
        disparity = F(uL - bestuR)                                  # :655
        why[iL] = 7
        if disparity >= minD and disparity < maxD:                  # :657-666
            why[iL] = 0
            if disparity <= 0:
                disparity = F(0.01)
                bestuR = F(np.float64(uL) - 0.01)
                why[iL] = 1
            mvDepth[iL] = F(F(mbf) / disparity)
            mvuRight[iL] = bestuR
            vDistIdx.append((bestDistS, iL))
    if not vDistIdx:          # the reference indexes an empty vector at :673; nothing to cut
        return mvuRight, mvDepth, 0, why
    vDistIdx.sort()                                                 # :672-685
    median = F(vDistIdx[len(vDistIdx) // 2][0])
    thDist = F(F(F(1.5) * F(1.4)) * median)
    valid = len(vDistIdx)
    for d, iL in reversed(vDistIdx):
        if F(d) < thDist:
            break
        mvuRight[iL] = -1
        mvDepth[iL] = -1
        why[iL] = 8
        valid -= 1
    return mvuRight, mvDepth, valid, why


# ---- 1. the oracle against the reading -------------------------------------------------------
DATASET_MBF, DATASET_FX = 386.1448, 718.856


def _levels(o):
    return [o.level(l) for l in range(o.nlevels)]


def _compare(oracle_mod, ol, orr, kL, dL, kR, dR, mbf, mb, what):
    from helpers import assert_f32_bits_equal
    tab = ol.tables()
    u_p, d_p, n_p, why_p = reference_stereo(kL, dL, kR, dR, _levels(ol), _levels(orr), tab["scale"],
                                            tab["inv_scale"], mbf, mb)
    u_o, d_o, n_o, why_o = oracle_mod.stereo_match(ol, orr, len(kL), mbf, mb, reasons=True)
    assert_f32_bits_equal(u_o, u_p, what + " uRight")
    assert_f32_bits_equal(d_o, d_p, what + " depth")
    assert n_o == n_p == int((u_p != -1).sum()), what
    assert np.array_equal(why_o, why_p), (what, np.nonzero(why_o != why_p)[0][:5])
    # reasons=False is the same function with reason == NULL
    u2, d2, n2 = oracle_mod.stereo_match(ol, orr, len(kL), mbf, mb)
    assert u2.tobytes() == u_o.tobytes() and d2.tobytes() == d_o.tobytes() and n2 == n_o
    return why_o


@pytest.fixture(scope="module")
def bases(oracle_mod):
    return sc.base_pairs(oracle_mod)


@pytest.fixture(scope="module")
def cases(bases):
    """{pair count: the cases of that batch}, exactly those of tests/test_gpu_stereo_directed.py."""
    return {B: sc.batch_cases(bases, B) for B in sorted(set(sc.REGIMES))}


def test_reading_equals_oracle_on_extracted_pairs(oracle_mod):
    """Four plain extracted pairs, with the datasets' maxD (718.9 px, wider than the image) and
    with the directed cases' (70.3 px)."""
    from my_orb_slam2_amd import synth
    ol, orr = oracle_mod.OracleExtractor(*sc.PARAMS), oracle_mod.OracleExtractor(*sc.PARAMS)
    mb_data = float(F(DATASET_MBF) / F(DATASET_FX))
    for i in range(4):
        L, R = synth.stereo_pair(60 + i, *sc.SIZE)
        kL, dL = ol(L)
        kR, dR = orr(R)
        for mb in (mb_data, sc.MB):
            why = _compare(oracle_mod, ol, orr, kL, dL, kR, dR, DATASET_MBF, mb, f"pair {i} mb={mb:.4f}")
            assert len(kL) >= 200 and (why == 0).sum() >= 70, (i, len(kL), np.bincount(why))


def test_reading_equals_oracle_on_injected_pairs(oracle_mod, bases, cases):
    """The 16 pairs of the 16-pair batch (11 regular over the four bases, the five special)."""
    kinds = set()
    for p, c in enumerate(cases[16]):
        b = bases[c.base]
        b["ol"].set_features(c.kL, c.dL)
        b["orr"].set_features(c.kR, c.dR)
        _compare(oracle_mod, b["ol"], b["orr"], c.kL, c.dL, c.kR, c.dR, sc.MBF, sc.MB,
                 f"injected pair {p} ({c.kind})")
        kinds.add(c.kind)
    assert kinds == {"regular", *sc.SPECIAL}


def test_set_features_restores(oracle_mod, bases):
    """set_features swaps features only: the pyramid stays, and putting the extracted features
    back gives the extracted pair's result again; a handle without an extraction refuses."""
    b = bases[1]
    lv = _levels(b["ol"])
    c = sc.generate(b, 1)
    b["ol"].set_features(c.kL, c.dL)
    b["orr"].set_features(c.kR, c.dR)
    injected = oracle_mod.stereo_match(b["ol"], b["orr"], len(c.kL), sc.MBF, sc.MB)
    assert all(np.array_equal(a, x) for a, x in zip(lv, _levels(b["ol"])))
    b["ol"].set_features(b["kL"], b["dL"])
    b["orr"].set_features(b["kR"], b["dR"])
    ol, orr = oracle_mod.OracleExtractor(*sc.PARAMS), oracle_mod.OracleExtractor(*sc.PARAMS)
    kL, _ = ol(b["imgL"])
    orr(b["imgR"])
    fresh = oracle_mod.stereo_match(ol, orr, len(kL), sc.MBF, sc.MB)
    back = oracle_mod.stereo_match(b["ol"], b["orr"], len(kL), sc.MBF, sc.MB)
    assert back[0].tobytes() == fresh[0].tobytes() and back[1].tobytes() == fresh[1].tobytes()
    assert back[2] == fresh[2] and back[2] >= 70
    assert injected[2] != back[2] or injected[0].tobytes() != back[0].tobytes()
    with pytest.raises(RuntimeError):
        oracle_mod.OracleExtractor(*sc.PARAMS).set_features(c.kL, c.dL)
    with pytest.raises(ValueError):
        b["ol"].set_features(c.kL, c.dL[:-1])


# ---- 2. coverage floors ----------------------------------------------------------------------
# Every exit and every directed construct at least FLOOR times in every batch of the GPU regime
# test.  Measured here, smallest count over the nine batches (it is the one-pair batch's every
# time) and the 129-pair batch's:
#   exit 0 accepted 56 / 12407, 1 clamped 15 / 474, 2 no candidate 20 / 2284, 3 filtered 79 / 8695,
#   4 distance in [75, 100) 91 / 9877, 5 SAD minimum at +-L 70 / 8638, 7 disparity 18 / 2336,
#   8 median cut 32 / 2052; best74 37 / 3785, best75 11 / 1429, best99 9 / 764,
#   tie_not_first 18 / 2057, at_minU 9 / 1510, at_maxU 16 / 1734.
# Exit 6 (deltaR outside [-1, 1]) has no floor: it cannot occur.  The SAD minimum d2 at an
# interior shift is strictly below the SADs before it and not above those after it, so with
# a = d1 - d2 > 0 and b = d3 - d2 >= 0 (exact integers in float32) deltaR = (a - b) / (2 (a + b))
# lies in [-0.5, 0.5] and is never NaN; the test asserts the oracle never reports it.  Exit 9
# (window outside the level) cannot occur for features that keep the border invariant.
FLOOR = 5
REACHABLE = (0, 1, 2, 3, 4, 5, 7, 8)


@pytest.mark.parametrize("B", sorted(set(sc.REGIMES)))
def test_coverage_floors(oracle_mod, bases, cases, B):
    counts = np.zeros(10, np.int64)
    cons = {}
    kinds = []
    for p, c in enumerate(cases[B]):
        assert c.base == p % 4 and c.kind == sc.pair_kind(B, p)
        kinds.append(c.kind)
        b = bases[c.base]
        b["ol"].set_features(c.kL, c.dL)
        b["orr"].set_features(c.kR, c.dR)
        u, d, n, why = oracle_mod.stereo_match(b["ol"], b["orr"], len(c.kL), sc.MBF, sc.MB, reasons=True)
        counts += np.bincount(why, minlength=10)
        assert n == int((u != -1).sum()) == int(((why == 0) | (why == 1)).sum())
        for name, idx in c.constructs.items():
            cons[name] = cons.get(name, 0) + len(idx)
            # what the generator planted is what the matcher met: a best distance of 75 or 99
            # ends at the distance test, one below 75 goes on to the SAD
            if name in ("best75", "best99"):
                assert (why[idx] == 4).all(), (p, name)
            else:
                assert not np.isin(why[idx], (2, 3, 4)).any(), (p, name)
        if c.kind == "full_cap":
            assert len(c.kL) == sc.KP_CAP
        if c.kind == "one_each":
            assert len(c.kL) == len(c.kR) == 1 and why[0] not in (2, 3, 4)   # its SAD ran
    print(f"B={B} exits {counts.tolist()} constructs {cons}")
    if B > 1:
        assert kinds[-5:] == list(sc.SPECIAL)
    assert counts[6] == 0 and counts[9] == 0, counts
    assert all(counts[c] >= FLOOR for c in REACHABLE), counts
    assert set(cons) == {"best74", "best75", "best99", "tie_not_first", "at_minU", "at_maxU"}
    assert all(v >= FLOOR for v in cons.values()), cons
