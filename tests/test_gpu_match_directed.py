"""GPU: the directed matcher cases (tests/matcher_cases.py) on the kernels of orbx_match.hip.

Every case goes through the single-call API and, where one exists, the batched device API;
matches and counts are bit-exact against the oracle (tests/test_oracle_match_directed.py has
checked the oracle on the same cases against a second restatement and against the outcome
each case states).  One ORBmatcher per (ratio, check_ori) serves all cases, in forward and
then in reverse order: the handle's scratch only grows, so a larger call must not leak into a
smaller one.  The size-regime tests take their sizes from orbx_matcher_variant and assert
the variant they mean to run before they run it.
"""
import numpy as np
import pytest

import matcher_cases as mc
from my_orb_slam2_amd import synth
from my_orb_slam2_amd.features import (PROJ_FRAME_MAPPOINTS, PROJ_LAST_FRAME, FeatureSet,
                                       assign_features_to_grid, feature_vector)

pytestmark = pytest.mark.gpu

S, S2, ISG = synth.scale_tables()
UNSUPPORTED, INVALID = -4, -1
MAX_FEAT = 32768
_matchers = {}


def matcher(ratio, ori):
    """The one ORBmatcher of this (ratio, check_ori), shared by every test of the module."""
    from my_orb_slam2_amd import ORBmatcher
    key = (float(ratio), bool(ori))
    if key not in _matchers:
        _matchers[key] = ORBmatcher(*key)
    return _matchers[key]


def ordered(cases, order):
    cases = sorted(cases, key=lambda c: c.name)
    return cases if order == "forward" else cases[::-1]


def T(gpu, a):
    import torch
    a = np.ascontiguousarray(a)
    b = a.view(np.uint8).reshape(-1) if a.size else np.zeros(16, np.uint8)
    return torch.from_numpy(b.copy()).to(gpu)


# ---- SearchByBoW ---------------------------------------------------------------------------

def bow_oracle(c):
    from oracle import matcher as om
    if c.kf_kf:
        return om.search_by_bow_kf_kf(c.a, c.va, c.b, c.vb, c.ratio, c.check_ori)
    return om.search_by_bow_kf_frame(c.a, c.va, c.b, c.ratio, c.check_ori)


def bow_gpu(c):
    m = matcher(c.ratio, c.check_ori)
    if c.kf_kf:
        return m.SearchByBoW(c.a, c.va, c.b, c.vb, f_is_keyframe=True)
    return m.SearchByBoW(c.a, c.va, c.b)


def bow_batch(c, gpu):
    """SearchByBoW(KeyFrame*, Frame&) through the batched device API (one keyframe)."""
    import torch
    from my_orb_slam2_amd.matcher import DeviceFeatureSet, DeviceKfDb
    m = matcher(c.ratio, c.check_ori)
    db, df = DeviceKfDb([c.a], [c.va], gpu), DeviceFeatureSet(c.b, gpu)
    out = torch.full((1, c.b.n), -7, dtype=torch.int32, device=gpu)
    cnt = torch.full((1,), -7, dtype=torch.int32, device=gpu)
    m.search_by_bow_kf_frame_batch_device(db.c, df.c, out, cnt)
    m.sync()
    return int(cnt.cpu()[0]), out.cpu().numpy()[0]


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_bow_cases(oracle_mod, orbx_lib, gpu, order):
    for c in ordered(mc.bow_cases(), order):
        n_o, m_o = bow_oracle(c)
        n_g, m_g = bow_gpu(c)
        assert n_g == n_o, c.name
        np.testing.assert_array_equal(m_g, m_o, err_msg=c.name)
        if not c.kf_kf:
            n_b, m_b = bow_batch(c, gpu)
            assert n_b == n_o, c.name
            np.testing.assert_array_equal(m_b, m_o, err_msg=c.name + " (batch)")


def _bow_regimes():
    from my_orb_slam2_amd.matcher import VK_BOW_KF_FRAME, VK_BOW_KF_KF, matcher_variant
    return {kf_kf: mc.scan_regimes(matcher_variant, VK_BOW_KF_KF if kf_kf else VK_BOW_KF_FRAME)
            for kf_kf in (False, True)}


@pytest.mark.parametrize("single_node", [True, False])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("kf_kf", [False, True])
def test_bow_size_regimes(oracle_mod, orbx_lib, gpu, kf_kf, variant, single_node):
    """The fullest LDS launch (the largest equal-sided size of k_bow<true>) and the smallest
    size of k_bow<false>, which reads the B descriptors from global memory."""
    from my_orb_slam2_amd.matcher import VK_BOW_KF_FRAME, VK_BOW_KF_KF, matcher_variant
    r = _bow_regimes()[kf_kf]
    n = r["first_fallback"] if variant else r["last_on_chip"]
    assert matcher_variant(VK_BOW_KF_KF if kf_kf else VK_BOW_KF_FRAME, n, n) == variant
    for check_ori in (False, True):
        c = mc.bow_regime_case(n, kf_kf, single_node, check_ori)
        m = matcher(c.ratio, c.check_ori)
        m.profile(True)
        n_g, m_g = bow_gpu(c)
        prof = m.collect_profile()
        m.profile(False)
        assert prof["k_bow"][1] == 1
        print(f"k_bow<{'false' if variant else 'true'}> n={n} kf_kf={kf_kf} single_node={single_node} "
              f"check_ori={check_ori}: {prof['k_bow'][0]:.3f} ms, {n_g} matches")
        n_o, m_o = bow_oracle(c)
        assert n_g == n_o and n_o > 100
        np.testing.assert_array_equal(m_g, m_o)
        if not kf_kf:
            n_b, m_b = bow_batch(c, gpu)
            assert n_b == n_o
            np.testing.assert_array_equal(m_b, m_o)


@pytest.mark.parametrize("kf_kf", [False, True])
def test_bow_first_unsupported_size(orbx_lib, gpu, kf_kf):
    from my_orb_slam2_amd import OrbxError
    r = _bow_regimes()[kf_kf]
    assert r["error"] == UNSUPPORTED
    c = mc.bow_regime_case(r["first_error"], kf_kf, True)
    with pytest.raises(OrbxError) as e:
        bow_gpu(c)
    assert e.value.code == UNSUPPORTED


# ---- SearchForTriangulation -----------------------------------------------------------------

def tri_oracle(c):
    from oracle import matcher as om
    return om.search_for_triangulation(c.k1, c.h1, c.k2, c.h2, c.F12, c.epi, S2, S,
                                       c.only_stereo, c.check_ori)


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_triangulation_cases(oracle_mod, orbx_lib, gpu, order):
    for c in ordered(mc.tri_cases(), order):
        n_o, p_o = tri_oracle(c)
        n_g, p_g = matcher(0.6, c.check_ori).SearchForTriangulation(
            c.k1, c.h1, c.k2, c.h2, c.F12, c.epi, S2, S, c.only_stereo)
        assert n_g == n_o, c.name
        np.testing.assert_array_equal(p_g, p_o, err_msg=c.name)


@pytest.mark.parametrize("node_order", [False, True])
@pytest.mark.parametrize("only_stereo,check_ori", [(False, False), (True, False), (False, True)])
def test_triangulation_cases_batch(oracle_mod, orbx_lib, gpu, only_stereo, check_ori, node_order):
    """The cases of one (only_stereo, check_ori) setting as the jobs of one batched call, in
    the plain database layout and in the node-order one."""
    import torch
    from my_orb_slam2_amd.matcher import DeviceKfDb
    cases = [c for c in ordered(mc.tri_cases(), "forward")
             if (c.only_stereo, c.check_ori) == (only_stereo, check_ori)]
    assert cases
    kfs, flags = [], []
    for c in cases:
        kfs += [c.k1, c.k2]
        flags += [c.h1, c.h2]
    m = matcher(0.6, check_ori)
    db = DeviceKfDb(kfs, flags, gpu)
    if node_order:
        db.node_order(m)
    jobs = np.arange(2 * len(cases), dtype=np.int32).reshape(-1, 2)
    job_off = np.concatenate([[0], np.cumsum([c.k1.n for c in cases])]).astype(np.int32)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    out = torch.full((int(job_off[-1]),), -7, dtype=torch.int32, device=gpu)
    cnt = torch.full((len(cases),), -7, dtype=torch.int32, device=gpu)
    m.search_for_triangulation_batch_device(
        db.c, tt(jobs[:, 0].copy()), tt(jobs[:, 1].copy()),
        tt(np.array([c.F12 for c in cases], np.float32)),
        tt(np.array([c.epi for c in cases], np.float32)), S2, S, tt(job_off), out, cnt,
        only_stereo=only_stereo)
    m.sync()
    out, cnt = out.cpu().numpy(), cnt.cpu().numpy()
    for j, c in enumerate(cases):
        n_o, p_o = tri_oracle(c)
        seg = out[job_off[j]:job_off[j + 1]]
        idx1 = np.nonzero(seg >= 0)[0]
        assert cnt[j] == n_o, c.name
        np.testing.assert_array_equal(np.stack([idx1, seg[idx1]], 1), p_o, err_msg=c.name)


# ---- projection searches --------------------------------------------------------------------

def proj_oracle(c, q=None, d=None):
    from oracle import matcher as om
    q, d = (c.q, c.qdesc) if q is None else (q, d)
    if c.qflags is None:
        return om.search_by_projection(c.mode, c.target, q, d, c.claimed, ISG,
                                       orb_dist=c.orb_dist, nnratio=c.ratio, check_ori=c.check_ori)
    return om.search_by_projection_ex(c.mode, c.target, q, d, c.qflags, c.claimed, ISG,
                                      orb_dist=c.orb_dist, nnratio=c.ratio, check_ori=c.check_ori,
                                      prefilter=c.prefilter)


def proj_gpu(c):
    m = matcher(c.ratio, c.check_ori)
    if c.qflags is None:
        return m.search_by_projection(c.mode, c.target, c.q, c.qdesc, c.claimed, ISG,
                                      orb_dist=c.orb_dist)
    return m.search_by_projection_ex(c.mode, c.target, c.q, c.qdesc, c.qflags, c.claimed, ISG,
                                     orb_dist=c.orb_dist, prefilter=c.prefilter)


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_projection_cases(oracle_mod, orbx_lib, gpu, order):
    for c in ordered(mc.proj_cases(), order):
        n_o, m_o = proj_oracle(c)
        n_g, m_g = proj_gpu(c)
        assert n_g == n_o >= 0, c.name
        np.testing.assert_array_equal(m_g, m_o, err_msg=c.name)


@pytest.mark.parametrize("mode", mc.ALL_MODES)
def test_projection_cases_batch(oracle_mod, orbx_lib, gpu, mode):
    """The mode's plain cases (one ratio / check_ori setting per call) as jobs of one batch,
    between empty jobs (first, last, two in a row), jobs of 1, 15, 16 and 17 queries (one
    16-query block of k_proj_search then spans jobs) and a job without target features."""
    import torch
    from my_orb_slam2_amd.matcher import DeviceFrameBatch
    plain = [c for c in ordered(mc.proj_cases(), "forward") if c.mode == mode and c.qflags is None]
    settings = sorted({(c.ratio, c.check_ori) for c in plain})
    assert settings
    for ratio, ori in settings:
        cases = [c for c in plain if (c.ratio, c.check_ori) == (ratio, ori)]
        first = cases[0]
        none = FeatureSet(first.target.keys[:0], first.target.desc[:0], first.target.u_right[:0],
                          feature_vector(np.zeros(0)), None)
        none.grid = assign_features_to_grid(none.keys, 0.0, mc.WIDTH, 0.0, mc.HEIGHT)
        # (target, queries, descriptors, claimed)
        jobs = [(first.target, first.q[:0], first.qdesc[:0], first.claimed)]
        for k in (1, 15, 16, 17):
            jobs.append((first.target, first.q[:k], first.qdesc[:k], first.claimed))
        jobs.append((first.target, first.q[:0], first.qdesc[:0], first.claimed))
        jobs.append((first.target, first.q[:0], first.qdesc[:0], first.claimed))
        jobs.append((none, first.q[:5], first.qdesc[:5], None))
        jobs += [(c.target, c.q, c.qdesc, c.claimed) for c in cases]
        jobs.append((first.target, first.q[:0], first.qdesc[:0], first.claimed))
        from oracle import matcher as om
        refs = [om.search_by_projection(mode, t, q, d, cl, ISG, orb_dist=mc.ORB_DIST,
                                        nnratio=ratio, check_ori=ori) for t, q, d, cl in jobs]
        m = matcher(ratio, ori)
        fb = DeviceFrameBatch([j[0] for j in jobs], gpu)
        q_off = np.concatenate([[0], np.cumsum([len(j[1]) for j in jobs])]).astype(np.int32)
        claimed = np.concatenate([np.zeros(t.n, np.uint8) if cl is None else cl.astype(np.uint8)
                                  for t, _, _, cl in jobs])
        out = torch.full((int(q_off[-1]),), -7, dtype=torch.int32, device=gpu)
        cnt = torch.full((len(jobs),), -7, dtype=torch.int32, device=gpu)
        m.search_by_projection_batch_device(
            mode, fb, T(gpu, np.concatenate([j[2] for j in jobs])),
            T(gpu, np.concatenate([j[1] for j in jobs])), torch.from_numpy(q_off).to(gpu), out,
            cnt, T(gpu, claimed), ISG, orb_dist=mc.ORB_DIST)
        m.sync()
        out, cnt = out.cpu().numpy(), cnt.cpu().numpy()
        for j, (n_o, m_o) in enumerate(refs):
            assert cnt[j] == n_o, (mode, ratio, ori, j)
            np.testing.assert_array_equal(out[q_off[j]:q_off[j + 1]], m_o, err_msg=f"job {j}")
        assert cnt.sum() > 0


def _proj_regimes(mode):
    from my_orb_slam2_amd.matcher import VK_PROJ, matcher_variant
    return mc.scan_regimes(matcher_variant, VK_PROJ + mode, nq=2000)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("ex", [False, True])
def test_projection_replay_regimes(oracle_mod, orbx_lib, gpu, ex, variant):
    """The claim replay with owner words at its largest target, and one query per round at
    MAX_FEAT, with about 2000 queries; plain FRAME_MAPPOINTS, and LAST_FRAME through the _ex
    entry point with no-claim queries and the prefilter."""
    from my_orb_slam2_amd.matcher import VK_PROJ, matcher_variant
    mode = PROJ_LAST_FRAME if ex else PROJ_FRAME_MAPPOINTS
    r = _proj_regimes(mode)
    n = MAX_FEAT if variant else r["last_on_chip"]
    assert r["first_fallback"] == r["last_on_chip"] + 1
    assert matcher_variant(VK_PROJ + mode, 0, n, 2000) == variant
    c = mc.proj_regime_case(n, mode, ex)
    assert c.target.n == n
    m = matcher(c.ratio, c.check_ori)
    m.profile(True)
    n_g, m_g = proj_gpu(c)
    prof = m.collect_profile()
    m.profile(False)
    assert prof["k_proj_resolve"][1] == 1
    print(f"k_proj_resolve variant {variant} target {n} ex={ex}: {prof['k_proj_resolve'][0]:.3f} ms, "
          f"{n_g} matches of {len(c.q)} queries")
    n_o, m_o = proj_oracle(c)
    assert n_g == n_o and n_o > 100
    np.testing.assert_array_equal(m_g, m_o)


def test_projection_target_above_max_feat(orbx_lib, gpu):
    from my_orb_slam2_amd import OrbxError
    from my_orb_slam2_amd.matcher import VK_PROJ, matcher_variant
    assert matcher_variant(VK_PROJ + PROJ_FRAME_MAPPOINTS, 0, MAX_FEAT + 1, 2000) == INVALID
    c = mc.proj_regime_case(MAX_FEAT + 1, PROJ_FRAME_MAPPOINTS, False)
    with pytest.raises(OrbxError) as e:
        proj_gpu(c)
    assert e.value.code == INVALID


# ---- SearchBySim3, SearchForInitialization, ComputeDistinctiveDescriptors --------------------

def test_sim3_directed(oracle_mod, orbx_lib, gpu):
    """SearchBySim3 on the SIM3 decisions case: its queries once more as KF1's features."""
    from oracle import matcher as om
    c = {c.name: c for c in mc.proj_cases()}["proj_sim3_decisions"]
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
    n_o, m_o = om.search_by_sim3(k1, k2, d1, q12, k2.desc, q21)
    n_g, m_g = matcher(0.8, False).SearchBySim3(k1, k2, d1, q12, k2.desc, q21)
    assert n_g == n_o > 0
    np.testing.assert_array_equal(m_g, m_o)


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_initialization_cases(oracle_mod, orbx_lib, gpu, order):
    from oracle import matcher as om
    for c in ordered(mc.init_cases(), order):
        p_g, p_o = c.prev.copy(), c.prev.copy()
        n_o, m_o = om.search_for_initialization(c.f1, c.f2, p_o, c.window, c.ratio, c.check_ori)
        n_g, m_g = matcher(c.ratio, c.check_ori).SearchForInitialization(c.f1, c.f2, p_g, c.window)
        assert n_g == n_o, c.name
        np.testing.assert_array_equal(m_g, m_o, err_msg=c.name)
        np.testing.assert_array_equal(p_g.view(np.int32), p_o.view(np.int32), err_msg=c.name)


INIT_LIMIT_SEED, INIT_LIMIT_WINDOW, INIT_LIMIT_PLANTS = 3, 30, 24


def init_limit_case(n):
    """(f1, f2, prev) with n features a side.  feature_pair gives every F2 feature at most one
    near F1 descriptor, so nothing is ever re-assigned; the case plants later (and, for the
    re-scan, earlier) exact copies of matched F2 descriptors into unmatched level-0 F1 features."""
    f1, f2, truth = synth.feature_pair(INIT_LIMIT_SEED, n1=n, n2=n)
    prev = np.ascontiguousarray(np.stack([f1.keys["x"], f1.keys["y"]], 1), np.float32)
    lvl0 = f1.keys["octave"] == 0
    free, held = np.nonzero(lvl0 & (truth < 0))[0], np.nonzero(lvl0 & (truth >= 0))[0]
    for k in range(INIT_LIMIT_PLANTS):
        i = held[len(held) // 4 + 7 * k]
        side = free[free > i] if k % 3 else free[free < i]
        i2, j = side[k], truth[i]
        f1.desc[i2] = f2.desc[j]
        prev[i2] = f2.keys["x"][j], f2.keys["y"][j]
    return f1, f2, prev


def test_initialization_at_lds_limit_between_claim_searches(oracle_mod, orbx_lib, gpu):
    """k_proj_init at the largest size its LDS carve allows (above 64 KiB: the kernel's raised
    dynamic-LDS limit is what lets it launch), between two k_proj_claim searches on the same
    handle."""
    import test_oracle_match as ref
    from my_orb_slam2_amd.matcher import VK_INIT, matcher_variant
    from oracle import matcher as om
    n = mc.scan_regimes(matcher_variant, VK_INIT)["last_on_chip"]
    assert 4 * (32 + 3 * n) > 64 * 1024 and matcher_variant(VK_INIT, n, n) == 0
    c = {c.name: c for c in mc.proj_cases()}["proj_frame_mappoints_claims"]
    assert c.mode == PROJ_FRAME_MAPPOINTS and c.qflags is None
    ratio, ori = c.ratio, True          # FRAME_MAPPOINTS has no rotation filter
    m = matcher(ratio, ori)

    def claim_search():
        n_o, m_o = om.search_by_projection(c.mode, c.target, c.q, c.qdesc, c.claimed, ISG,
                                           orb_dist=c.orb_dist, nnratio=ratio, check_ori=ori)
        n_g, m_g = m.search_by_projection(c.mode, c.target, c.q, c.qdesc, c.claimed, ISG,
                                          orb_dist=c.orb_dist)
        assert n_g == n_o > 0
        np.testing.assert_array_equal(m_g, m_o)

    f1, f2, prev = init_limit_case(n)
    p_g, p_o, p_r = prev.copy(), prev.copy(), prev.copy()
    n_o, m_o = om.search_for_initialization(f1, f2, p_o, INIT_LIMIT_WINDOW, ratio, ori)
    codes = ref.initialization_py(f1, f2, p_r, INIT_LIMIT_WINDOW, ratio, ori)[2]
    rescans = sum("+rescan" in k for k in codes)
    print(f"n={n}: {n_o} matches, {codes.count('taken_over')} re-assigned, {rescans} re-scans, "
          f"{codes.count('rotation_removed')} rotated out")
    assert n_o > 100 and codes.count("taken_over") >= 1 and rescans >= 1   # CPU run: 943, 8, 382
    claim_search()
    n_g, m_g = m.SearchForInitialization(f1, f2, p_g, INIT_LIMIT_WINDOW)
    claim_search()
    assert n_g == n_o
    np.testing.assert_array_equal(m_g, m_o)
    np.testing.assert_array_equal(p_g.view(np.int32), p_o.view(np.int32))


def test_initialization_first_unsupported_size(orbx_lib, gpu):
    from my_orb_slam2_amd import OrbxError
    from my_orb_slam2_amd.matcher import VK_INIT, matcher_variant
    r = mc.scan_regimes(matcher_variant, VK_INIT)
    assert r["error"] == UNSUPPORTED
    n = r["first_error"]
    f1, f2, _ = synth.feature_pair(3, n1=n, n2=n)
    prev = np.ascontiguousarray(np.stack([f1.keys["x"], f1.keys["y"]], 1), np.float32)
    with pytest.raises(OrbxError) as e:
        matcher(0.9, True).SearchForInitialization(f1, f2, prev, 10)
    assert e.value.code == UNSUPPORTED


def test_distinctive_directed(oracle_mod, orbx_lib, gpu):
    from my_orb_slam2_amd import OrbxError
    from oracle import matcher as om
    desc, off, expect = mc.distinctive_case()
    m = matcher(0.6, True)
    got = m.compute_distinctive_descriptors(desc, off)
    np.testing.assert_array_equal(got, om.distinctive_descriptors(desc, off))
    np.testing.assert_array_equal(got, expect)
    big = np.concatenate([desc[:1]] * 257)
    with pytest.raises(OrbxError) as e:
        m.compute_distinctive_descriptors(big, np.array([0, 257], np.int32))
    assert e.value.code == UNSUPPORTED
    # a smaller call after a larger one on the same handle
    np.testing.assert_array_equal(m.compute_distinctive_descriptors(desc[:3], off[:4]), expect[:3])
    # the device entry point: a point above the limit gets -1 and is flagged at the sync
    import torch
    from my_orb_slam2_amd._lib import check, ptr
    off2 = np.concatenate([off, [off[-1] + 257]]).astype(np.int32)
    d_desc, d_off = T(gpu, np.concatenate([desc, big])), torch.from_numpy(off2).to(gpu)
    d_best = torch.full((len(off2) - 1,), -7, dtype=torch.int32, device=gpu)
    check("orbx_compute_distinctive_descriptors_device",
          m._lib.orbx_compute_distinctive_descriptors_device(m._h, ptr(d_desc), ptr(d_off),
                                                             len(off2) - 1, ptr(d_best), None))
    with pytest.raises(OrbxError):
        m.sync()
    np.testing.assert_array_equal(d_best.cpu().numpy(), np.concatenate([expect, [-1]]))
