"""CPU: the directed matcher cases (tests/matcher_cases.py) through the oracle and through the
plain-Python restatements of tests/test_oracle_match.py.

Three things are asserted here, all without a GPU:
  * the oracle and the restatement agree bit for bit on every small case (matches, counts
    and, for SearchForInitialization, vbPrevMatched), non-finite and huge queries included;
  * every probe of a case has the outcome and the match the case states, so each planted
    boundary has a case on either side whose outcome differs because of that boundary alone;
  * the coverage floors: every outcome code occurs for every matcher and mode it applies to,
    the replay's structural edges occur, and orbx_matcher_variant reaches both variants.
These are conditions on the inputs, met by the reference behaviour alone: the GPU test
(tests/test_gpu_match_directed.py) imports the very same cases.
"""
from __future__ import annotations

import numpy as np
import pytest

import matcher_cases as mc
import test_oracle_match as ref
from my_orb_slam2_amd import synth
from my_orb_slam2_amd.features import (PROJ_FRAME_MAPPOINTS, PROJ_KEYFRAME, PROJ_LAST_FRAME,
                                       PROJ_SIM3)
from oracle import matcher as om

BOW = {c.name: c for c in mc.bow_cases()}
TRI = {c.name: c for c in mc.tri_cases()}
PROJ = {c.name: c for c in mc.proj_cases()}
INIT = {c.name: c for c in mc.init_cases()}
S, S2, ISG = synth.scale_tables()

UNSUPPORTED, INVALID = -4, -1
MAX_FEAT = 32768


def check_probes(case, codes, matched):
    """matched(index) -> the match of probe `index` in the result under test."""
    for p in case.probes:
        assert codes[p.index] == p.expect, (case.name, p, codes[p.index])
        if p.match is not None:
            assert matched(p.index) == p.match, (case.name, p, matched(p.index))


# ---- SearchByBoW ---------------------------------------------------------------------------

def bow_oracle(c):
    if c.kf_kf:
        return om.search_by_bow_kf_kf(c.a, c.va, c.b, c.vb, c.ratio, c.check_ori)
    return om.search_by_bow_kf_frame(c.a, c.va, c.b, c.ratio, c.check_ori)


def bow_match_of(c, m):
    """The B feature matched to A feature i (the KF-F result is indexed by B feature)."""
    if c.kf_kf:
        return lambda i: int(m[i])
    inv = {int(a): j for j, a in enumerate(m) if a >= 0}
    return lambda i: inv.get(i, -1)


@pytest.mark.parametrize("name", sorted(BOW))
def test_bow_case(oracle_mod, name):
    c = BOW[name]
    n_o, m_o = bow_oracle(c)
    n_p, m_p, codes = ref.bow_py(c.a, c.va, c.b, c.vb, c.kf_kf, c.ratio, c.check_ori)
    assert n_o == n_p
    np.testing.assert_array_equal(m_o, m_p)
    assert c.probes
    check_probes(c, codes, bow_match_of(c, m_o))


def test_bow_float_ratio_edges():
    """The ratio test runs in float32: 30 < 0.6f * 50 holds (30.000002), 9 < 0.6f * 15 does not
    (the product rounds to 9.0, in double it is 9.0000004); 30 < 0.75f * 40 is an exact tie."""
    assert mc.ratio_accepts(30, 50, 0.6) and not 30 < 0.6 * 50
    assert not mc.ratio_accepts(9, 15, 0.6) and 9 < float(np.float32(0.6)) * 15
    assert not mc.ratio_accepts(30, 40, 0.75) and not mc.ratio_accepts(45, 50, 0.9)
    assert (9, 15) in mc.float_double_disagreements(0.6, True, 50)
    for fl in ("kff", "kfkf"):
        c = BOW[f"bow_{fl}_decisions_r0.6"]
        why = {p.why: p.expect for p in c.probes}
        assert why["ratio 0.6: 30/50"] == "accepted" and why["ratio 0.6: 31/50"] == "ratio_rejected"
        assert why["ratio 0.6: 9/15"] == "ratio_rejected" and why["ratio 0.6: 8/15"] == "accepted"
        assert why["best 49, far second"] == "accepted" and why["best 51, far second"] == "over_threshold"
        assert why["best 50, far second"] == ("over_threshold" if fl == "kfkf" else "accepted")
        c = BOW[f"bow_{fl}_decisions_r0.75"]
        why = {p.why: p.expect for p in c.probes}
        assert why["ratio 0.75: 30/40"] == "ratio_rejected" and why["ratio 0.75: 29/40"] == "accepted"
        c = BOW[f"bow_{fl}_decisions_r0.9"]
        why = {p.why: p.expect for p in c.probes}
        assert why["ratio 0.9: 45/50"] == "ratio_rejected" and why["ratio 0.9: 44/50"] == "accepted"


def test_three_maxima_float_edges():
    """0.1f * max1 in float32 keeps a second or third bin of exactly a tenth (1 of 10, 2 of 20,
    10 of 100); in double 0.1f is above 0.1 and the bin would be dropped."""
    for m1, m2 in ((10, 1), (20, 2), (100, 10)):
        assert not m2 < np.float32(0.1) * np.float32(m1)
        assert m2 < float(np.float32(0.1)) * m1
        assert om.three_maxima([m1, m2] + [0] * 28) == (0, 1, -1)
        assert om.three_maxima([m1, m2, m2] + [0] * 27) == (0, 1, 2)
    assert om.three_maxima([100, 9] + [0] * 28) == (0, -1, -1)
    assert om.three_maxima([100, 10, 9] + [0] * 27) == (0, 1, -1)
    assert om.three_maxima([4, 4, 4, 4] + [0] * 26) == (0, 1, 2)


# ---- SearchForTriangulation -----------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(TRI))
def test_triangulation_case(oracle_mod, name):
    c = TRI[name]
    n_o, p_o = om.search_for_triangulation(c.k1, c.h1, c.k2, c.h2, c.F12, c.epi, S2, S,
                                           c.only_stereo, c.check_ori)
    codes = []
    n_p, p_p = ref.triangulation_py(c.k1, c.h1, c.k2, c.h2, c.F12, c.epi[0], c.epi[1], S2, S,
                                    c.only_stereo, c.check_ori, codes)
    assert n_o == n_p
    np.testing.assert_array_equal(p_o, p_p)
    got = {int(a): int(b) for a, b in p_o}
    assert c.probes
    check_probes(c, codes, lambda i: got.get(i, -1))


# ---- projection searches --------------------------------------------------------------------

def proj_oracle(c):
    if c.qflags is None:
        return om.search_by_projection(c.mode, c.target, c.q, c.qdesc, c.claimed, ISG,
                                       orb_dist=c.orb_dist, nnratio=c.ratio, check_ori=c.check_ori)
    return om.search_by_projection_ex(c.mode, c.target, c.q, c.qdesc, c.qflags, c.claimed, ISG,
                                      orb_dist=c.orb_dist, nnratio=c.ratio, check_ori=c.check_ori,
                                      prefilter=c.prefilter)


def proj_restated(c):
    info = {}
    n, m = ref.projection_py(c.mode, c.target, c.q, c.qdesc, c.claimed, c.ratio, c.check_ori,
                             orb_dist=c.orb_dist, inv_sigma2=ISG, qflags=c.qflags,
                             prefilter=c.prefilter, info=info)
    return n, m, info


@pytest.mark.parametrize("name", sorted(PROJ))
def test_projection_case(oracle_mod, name):
    c = PROJ[name]
    n_o, m_o = proj_oracle(c)
    n_p, m_p, info = proj_restated(c)
    assert n_o == n_p >= 0
    np.testing.assert_array_equal(m_o, m_p)
    assert c.probes
    # a no-claim query's match may be stated although a later query takes the same feature
    check_probes(c, info["codes"], lambda i: int(m_o[i]))


def test_projection_replay_floors(oracle_mod):
    """The claims cases exhaust a truncated candidate list in chunk 0 and in a later chunk
    (also at lanes 0, 1 and 63), decide a list of exactly 8 without one, and the no-claim cases
    have a no-claim query whose feature a later query takes."""
    for mode in mc.CLAIM_MODES:
        nm = mc.MODE_NAME[mode]
        for suffix in ("claims", "claims_ex"):
            c = PROJ[f"proj_{nm}_{suffix}"]
            assert len(c.q) == 129
            ex = proj_restated(c)[2]["exhausted"]
            assert {8, 63, 64, 65, 127} <= set(ex), (c.name, ex)
            exact8 = [p.index for p in c.probes if p.why.startswith("list of exactly 8")]
            assert exact8 and exact8[0] not in ex
        c = PROJ[f"proj_{nm}_no_claim"]
        over = proj_restated(c)[2]["overwritten"]
        assert bool(over) == (mode in (PROJ_FRAME_MAPPOINTS, PROJ_LAST_FRAME)), (c.name, over)
        if over:
            assert 63 in over    # taken by the first query of the next chunk
        for nq in (63, 64, 65):
            assert len(PROJ[f"proj_{nm}_claims_nq{nq}"].q) == nq


def test_projection_float_ratio_edges():
    """FRAME_MAPPOINTS' bestDist > ratio * bestDist2 in float32: no (d1, d2) separates float
    from double for 0.8f (which lies above 0.8, so the rounded product never crosses an
    integer from the side that matters); for 0.9f, 45 > 0.9f * 50 is false in float32 (the
    product rounds to 45.0) and true in double, so a ratio 0.9 case carries that pair."""
    assert mc.float_double_disagreements(0.8, False) == []
    assert (45, 50) in mc.float_double_disagreements(0.9, False)
    why = {p.why: p.expect for p in PROJ["proj_frame_mappoints_decisions_r0.9"].probes}
    assert why["45/50 ratio 0.9 same level"] == "accepted"
    assert why["46/50 ratio 0.9 same level"] == "ratio_rejected"
    assert why["46/50 ratio 0.9 other level"] == "accepted"
    why = {p.why: p.expect for p in PROJ["proj_frame_mappoints_decisions"].probes}
    assert why["40/50 ratio 0.8 same level"] == "accepted"      # an exact tie: > is strict
    assert why["41/50 ratio 0.8 same level"] == "ratio_rejected"


def test_sim3_mutual_check(oracle_mod):
    """SearchBySim3 on the SIM3 decisions case in both directions: KF2's features as queries
    into KF1 = the case's own queries as features."""
    c = PROJ["proj_sim3_decisions"]
    k2 = c.target
    ok = np.nonzero(np.isfinite(c.q["u"]) & np.isfinite(c.q["v"]))[0]
    s = mc._Set()
    for i in ok:
        s.add(c.qdesc[i], -1, x=float(np.clip(c.q["u"][i], 0, 740)),
              y=float(np.clip(c.q["v"][i], 0, 470)), octave=0)
    k1 = s.build()
    q12, d1 = c.q[ok], c.qdesc[ok]
    q21 = np.zeros(k2.n, c.q.dtype)
    q21["u"], q21["v"], q21["radius"] = k2.keys["x"], k2.keys["y"], 8.0
    q21["pred_level"] = 0
    n_o, m_o = om.search_by_sim3(k1, k2, d1, q12, k2.desc, q21)
    n_p, m_p = ref.sim3_py(k1, k2, d1, q12, k2.desc, q21)
    assert n_o == n_p > 0
    np.testing.assert_array_equal(m_o, m_p)
    one_way = ref.projection_py(PROJ_SIM3, k2, q12, d1, None, 0.0, False)[1]
    assert ((one_way >= 0) & (m_o < 0)).any()      # the mutual check removes something


# ---- SearchForInitialization ----------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(INIT))
def test_initialization_case(oracle_mod, name):
    c = INIT[name]
    p_o, p_p = c.prev.copy(), c.prev.copy()
    n_o, m_o = om.search_for_initialization(c.f1, c.f2, p_o, c.window, c.ratio, c.check_ori)
    n_p, m_p, codes = ref.initialization_py(c.f1, c.f2, p_p, c.window, c.ratio, c.check_ori)
    assert n_o == n_p
    np.testing.assert_array_equal(m_o, m_p)
    np.testing.assert_array_equal(p_o.view(np.int32), p_p.view(np.int32))
    check_probes(c, codes, lambda i: int(m_o[i]))
    # vbPrevMatched moves for the matched features only
    moved = (p_o.view(np.int32) != c.prev.view(np.int32)).any(1)
    assert moved.any() and not moved[m_o < 0].any() and moved[m_o >= 0].all()


# ---- ComputeDistinctiveDescriptors -----------------------------------------------------------

def test_distinctive_case(oracle_mod):
    desc, off, expect = mc.distinctive_case()
    assert sorted(np.diff(off)) == [0, 1, 2, 3, 4, 5, 6, 63, 64, 65, 256]
    np.testing.assert_array_equal(om.distinctive_descriptors(desc, off), expect)
    np.testing.assert_array_equal(ref.distinctive_py(desc, off), expect)


# ---- coverage floors -------------------------------------------------------------------------

def _codes_of(cases, run):
    out = set()
    for c in cases:
        out |= set(run(c))
    return out


def test_outcome_code_floors(oracle_mod):
    """Every outcome code occurs at least once for every matcher and mode it applies to.
    A "skipped+rescan" cannot occur (a skipped feature looks at no candidate), and neither can
    a KF-F "no_candidate" without "+rescan": a shared node has a B feature, and before the
    first claim nothing keeps it from being a candidate."""
    base = {"skipped", "no_candidate", "over_threshold", "ratio_rejected", "accepted"}
    for kf_kf in (False, True):
        got = _codes_of([c for c in BOW.values() if c.kf_kf == kf_kf],
                        lambda c: ref.bow_py(c.a, c.va, c.b, c.vb, c.kf_kf, c.ratio, c.check_ori)[2])
        assert got >= (base - {"no_candidate"}) | {"rotation_removed", "accepted+rescan",
                                                    "no_candidate+rescan", "over_threshold+rescan"}, got
        assert ("no_candidate" in got) == kf_kf
        assert not any(g.startswith("skipped+") for g in got)

    def tri(c):
        codes = []
        ref.triangulation_py(c.k1, c.h1, c.k2, c.h2, c.F12, c.epi[0], c.epi[1], S2, S,
                             c.only_stereo, c.check_ori, codes)
        return codes
    assert _codes_of(TRI.values(), tri) == {"skipped", "no_candidate", "accepted", "rotation_removed"}
    for mode in mc.ALL_MODES:
        got = _codes_of([c for c in PROJ.values() if c.mode == mode],
                        lambda c: proj_restated(c)[2]["codes"])
        want = {"skipped", "no_candidate", "over_threshold", "accepted"}
        if mode == PROJ_FRAME_MAPPOINTS:
            want |= {"ratio_rejected"}
        if mode in mc.CLAIM_MODES:
            want |= {"accepted+rescan", "no_candidate+rescan"}
        if mode in (PROJ_LAST_FRAME, PROJ_KEYFRAME):
            want |= {"rotation_removed"}
        assert got >= want, (mode, got)
        if mode not in mc.CLAIM_MODES:
            assert not any("+rescan" in g for g in got), (mode, got)
        if mode != PROJ_FRAME_MAPPOINTS:
            assert "ratio_rejected" not in got
    got = _codes_of(INIT.values(), lambda c: ref.initialization_py(
        c.f1, c.f2, c.prev.copy(), c.window, c.ratio, c.check_ori)[2])
    assert got >= base | {"taken_over", "rotation_removed", "accepted+rescan", "no_candidate+rescan"}, got


# ---- orbx_matcher_variant and the size regimes -------------------------------------------------

def test_variant_query_reaches_both_variants(orbx_lib):
    """Host only.  The first fallback size is found by scanning; the formula's values (LDS at
    3395, global from 3396, unsupported from 10135; owner words up to 32688) are what the
    scan must find, so a change of the LDS carve shows up here."""
    from my_orb_slam2_amd.matcher import (VK_BOW_KF_FRAME, VK_BOW_KF_KF, VK_INIT, VK_PROJ,
                                          matcher_variant)
    for kind in (VK_BOW_KF_FRAME, VK_BOW_KF_KF):
        r = mc.scan_regimes(matcher_variant, kind)
        assert r["last_on_chip"] is not None and r["first_fallback"] == r["last_on_chip"] + 1
        assert r["error"] == UNSUPPORTED and r["first_error"] > r["first_fallback"]
        assert (r["last_on_chip"], r["first_error"]) == (3395, 10135)
        assert matcher_variant(kind, MAX_FEAT + 1, 1) == INVALID
        assert matcher_variant(kind, 1, -1) == INVALID
    for mode in mc.ALL_MODES:
        r = mc.scan_regimes(matcher_variant, VK_PROJ + mode, nq=2000)
        assert (r["first_error"], r["error"]) == (MAX_FEAT + 1, INVALID)
        if mode in mc.CLAIM_MODES:
            assert r["first_fallback"] == r["last_on_chip"] + 1 <= MAX_FEAT
            assert matcher_variant(VK_PROJ + mode, 0, MAX_FEAT, 2000) == 1
        else:
            assert r["first_fallback"] is None and r["last_on_chip"] == MAX_FEAT
    r = mc.scan_regimes(matcher_variant, VK_INIT)
    assert r["first_fallback"] is None and r["error"] == UNSUPPORTED
    assert r["first_error"] == r["last_on_chip"] + 1
    assert (r["last_on_chip"], r["first_error"]) == (13621, 13622)   # 4 * (32 + 3n) bytes of LDS
    assert matcher_variant(VK_PROJ + 7, 0, 10, 10) == INVALID
    assert matcher_variant(VK_PROJ - 1, 0, 10, 10) == INVALID


@pytest.mark.parametrize("single_node", [True, False])
@pytest.mark.parametrize("kf_kf", [False, True])
def test_bow_regime_case_probes(oracle_mod, kf_kf, single_node):
    """The regime cases' planted claim chain, through the oracle alone (pure Python is too
    slow at this size); the size here only has to be large, the GPU test takes it from
    orbx_matcher_variant."""
    c = mc.bow_regime_case(3396, kf_kf, single_node)
    n_o, m_o = bow_oracle(c)
    of = bow_match_of(c, m_o)
    assert n_o > 100 and len(c.probes) == 4
    for p in c.probes:
        assert of(p.index) == p.match, p
    assert not mc.bow_regime_case(3396, kf_kf, single_node, True).probes


@pytest.mark.parametrize("ex", [False, True])
def test_projection_regime_case_probes(oracle_mod, ex):
    c = mc.proj_regime_case(MAX_FEAT, PROJ_LAST_FRAME if ex else PROJ_FRAME_MAPPOINTS, ex)
    assert c.target.n == MAX_FEAT and 1900 <= len(c.q) <= 2100
    n_o, m_o = proj_oracle(c)
    assert n_o > 100
    for p in c.probes:
        assert int(m_o[p.index]) == p.match, p
