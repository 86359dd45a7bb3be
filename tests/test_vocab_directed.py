"""Directed vocabulary cases (tests/vocab_cases.py).
CPU: OracleVocabulary equals the independent transform_py reading of test_vocab.py on every
case, the census of the construct names, and the load error that needs no device.
GPU: the library equals the oracle on every case (words, nodes, BowVector bit for bit,
FeatureVector), orbx_vocabulary_transform_device gives transform's words and nodes on device
tensors, and k_bow_score (host and device entry points) equals the restated L1 score at every
shape, up to orbx_bow_db_score_max_query() and not one word further."""
import ctypes

import numpy as np
import pytest

import vocab_cases as vc
from test_vocab import transform_py
from vocab_cases import CASES

IDS = [c["name"] for c in CASES]
OK, ERR_INVALID, ERR_UNSUPPORTED = 0, -1, -4


def _write(tmp_path, case):
    p = tmp_path / (case["name"] + ".txt")
    p.write_bytes(case["text"].encode())
    return p


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_equals_python_reading(tmp_path, oracle_mod, case):
    from oracle.matcher import OracleVocabulary
    path = _write(tmp_path, case)
    v = OracleVocabulary(path)
    for lu in case["levelsups"]:
        w, n, (bw, bv), (fn, fo, ff) = v.transform(case["desc"], lu)
        pw, pn, pbow, pfv = transform_py(path, case["desc"], lu)
        keys = sorted(pbow)
        np.testing.assert_array_equal(w, np.array(pw, np.int32))
        np.testing.assert_array_equal(n, np.array(pn, np.int32))
        np.testing.assert_array_equal(bw, np.array(keys, np.uint32))
        np.testing.assert_array_equal(bv.view(np.int64),
                                      np.array([pbow[a] for a in keys], np.float64).view(np.int64))
        np.testing.assert_array_equal(fn, np.array(sorted(pfv), np.uint32))
        np.testing.assert_array_equal(
            ff, np.concatenate([pfv[a] for a in sorted(pfv)]) if pfv else np.zeros(0, np.int32))
        np.testing.assert_array_equal(fo, np.cumsum([0] + [len(pfv[a]) for a in sorted(pfv)]))


def test_planted_outcomes(tmp_path, oracle_mod):
    """What the cases say they plant, read off the oracle."""
    from oracle.matcher import OracleVocabulary
    by = {c["name"]: c for c in CASES}

    def words(name, lu=0):
        c = by[name]
        return [list(x) for x in OracleVocabulary(_write(tmp_path, c)).transform(c["desc"], lu)[:2]]

    assert words("tie_children_0_1")[0][:2] == [0, 0]
    assert words("tie_children_0_last")[0][:2] == [0, 0]
    assert words("tie_children_last_two")[0][:2] == [2, 2]
    assert words("tie_all_children")[0] == [0] * 6
    assert words("tie_different_bits")[0] == [0, 0, 2, 1]
    assert words("distance_0_and_256")[0][:2] == [1, 0]
    for g in range(4):
        assert words(f"bytes_{8 * g}_{8 * g + 7}")[0] == [2 * i + 1 for i in range(8)]
    # ragged: leaf depths 1 / 2 / 3, the childless isLeaf-0 node (word 0, node 8), one child
    w, n = words("ragged", 0)            # nid_level 3: shallower leaves report themselves
    assert w[:8] == [0, 0, 1, 3, 4, 3, 0, 2] and n[:8] == [1, 1, 4, 7, 9, 7, 8, 5]
    w, n = words("ragged", 2)            # nid_level 1
    assert n[:8] == [1, 1, 2, 2, 2, 2, 2, 3]
    assert set(words("ragged", 3)[1]) == {0} and set(words("ragged", 6)[1]) == {0}
    assert words("ragged", -1)[1][:8] == [1, 1, 4, 7, 9, 7, 8, 5]   # a level never reached
    assert words("ragged_crlf_blank", 0) == words("ragged", 0)
    assert set(words("k1_chain")[0]) == {0} and set(words("k1_chain", 1)[1]) == {2}
    c = by["stop_word_third"]
    v = OracleVocabulary(_write(tmp_path, c))
    w, _, (bw, bv), (fn, fo, ff) = v.transform(c["desc"], 0)
    assert list(w).count(1) == 10 and list(bw) == [0, 2] and len(ff) == 20
    for sc in (0, 1, 5):
        c = by[f"all_stop_words_sc{sc}"]
        _, _, (bw, bv), (fn, fo, ff) = OracleVocabulary(_write(tmp_path, c)).transform(c["desc"], 0)
        assert len(bw) == 0 and len(fn) == 0 and list(fo) == [0]


def test_census_constructs():
    planted = [x for c in CASES for x in c["constructs"]]
    assert sorted(set(planted)) == sorted(vc.CONSTRUCTS)
    assert {c["levelsups"] for c in CASES if "levelsup_sweep" in c["constructs"]} == {(-1, 0, 1, 2, 3, 6)}


def test_bad_parent_is_invalid(tmp_path, orbx_lib):
    """parent >= own id: ORBX_ERR_INVALID, decided before any device call."""
    for i, txt in enumerate(vc.BAD_PARENT):
        p = tmp_path / f"bad{i}.txt"
        p.write_text(txt)
        h = ctypes.c_void_p()
        assert orbx_lib.orbx_vocabulary_load_text(str(p).encode(), 0, ctypes.byref(h)) == ERR_INVALID
        assert not h.value


def test_max_query_is_the_launcher_limit(orbx_lib):
    """The LDS of k_bow_score: 4 nq (rounded to 8) + 8 (nq + 256) bytes within 64 KiB."""
    m = orbx_lib.orbx_bow_db_score_max_query()
    lds = lambda nq: ((4 * nq + 7) & ~7) + 8 * (nq + 256)
    assert lds(m) <= 65536 < lds(m + 1)


# ---- GPU -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gpu_vocab_equals_oracle(tmp_path, oracle_mod, orbx_lib, gpu, case):
    import torch
    from my_orb_slam2_amd import Vocabulary
    from my_orb_slam2_amd._lib import ptr
    from oracle.matcher import OracleVocabulary
    path = _write(tmp_path, case)
    gv, ov = Vocabulary.load_text(path), OracleVocabulary(path)
    d = case["desc"]
    n = len(d)
    for lu in case["levelsups"]:
        w, nd, (bw, bv), fv = gv.transform(d, lu)
        ow, on, (obw, obv), (ofn, ofo, off) = ov.transform(d, lu)
        np.testing.assert_array_equal(w, ow)
        np.testing.assert_array_equal(nd, on)
        np.testing.assert_array_equal(bw, obw)
        np.testing.assert_array_equal(bv.view(np.int64), obv.view(np.int64))
        np.testing.assert_array_equal(fv.node_id, ofn)
        np.testing.assert_array_equal(fv.off, ofo)
        np.testing.assert_array_equal(fv.feat, off)
        # the descent alone on device tensors (word ids straight from the kernel)
        td = torch.from_numpy(d.copy()).to(gpu) if n else torch.zeros((1, 32), dtype=torch.uint8, device=gpu)
        tw = torch.full((max(n, 1),), -7, dtype=torch.int32, device=gpu)
        tn = torch.full((max(n, 1),), -7, dtype=torch.int32, device=gpu)
        torch.cuda.synchronize()
        assert orbx_lib.orbx_vocabulary_transform_device(gv._h, ptr(td), n, lu, ptr(tw), ptr(tn),
                                                         None) == OK
        torch.cuda.synchronize()
        np.testing.assert_array_equal(tw.cpu().numpy()[:n], ow)
        np.testing.assert_array_equal(tn.cpu().numpy()[:n], on)
        if n == 0:
            assert int(tw[0]) == -7 and int(tn[0]) == -7   # nothing written


@pytest.mark.gpu
def test_gpu_header_only_vocabulary(tmp_path, orbx_lib, gpu):
    """empty() (TemplatedVocabulary.h:1134): both vectors empty.  Not run through the oracle,
    which would index an empty child list."""
    from my_orb_slam2_amd import Vocabulary
    p = tmp_path / "empty.txt"
    p.write_text(vc.HEADER_ONLY)
    v = Vocabulary.load_text(p)
    assert (v.n_nodes, v.n_words) == (1, 0)
    w, n, (bw, bv), fv = v.transform(vc.rand_desc(np.random.default_rng(0), 5), 4)
    assert len(bw) == 0 and len(fv.node_id) == 0 and list(fv.off) == [0]


def _expected_scores(q, kfs):
    from oracle.matcher import bow_score_l1 as o_score
    common = np.array([len(np.intersect1d(q[0], b[0])) for b in kfs], np.int32)
    score = np.array([np.float32(o_score(q, b)) for b in kfs], np.float32)
    return common, score


def _flat(kfs, lead):
    """Concatenated keyframe vectors behind `lead` filler entries (kf_off[0] = lead)."""
    off = np.zeros(len(kfs) + 1, np.int32)
    off[0] = lead
    np.cumsum([len(b[0]) for b in kfs], out=off[1:])
    off[1:] += lead
    words = np.concatenate([np.full(lead, 7, np.uint32)] + [np.asarray(b[0], np.uint32) for b in kfs])
    vals = np.concatenate([np.full(lead, 0.25)] + [np.asarray(b[1], np.float64) for b in kfs])
    return off, np.ascontiguousarray(words), np.ascontiguousarray(vals)


@pytest.mark.gpu
@pytest.mark.parametrize("name,q,kfs", vc.bow_score_sets(), ids=[s[0] for s in vc.bow_score_sets()])
@pytest.mark.parametrize("lead", [0, 5])
def test_gpu_bow_db_score_directed(oracle_mod, orbx_lib, gpu, name, q, kfs, lead):
    import torch
    from my_orb_slam2_amd._lib import ptr
    want_c, want_s = _expected_scores(q, kfs)
    if name == "order_dependent_sum":
        assert want_s[0] == np.float32(2.0**52) and want_s[2] == np.float32(2.0**52)
    qw, qv = np.ascontiguousarray(q[0], np.uint32), np.ascontiguousarray(q[1], np.float64)
    off, words, vals = _flat(kfs, lead)
    nkf = len(kfs)
    common, score = np.full(nkf, -7, np.int32), np.full(nkf, -7, np.float32)
    assert orbx_lib.orbx_bow_db_score(ptr(qw), ptr(qv), len(qw), nkf, ptr(off), ptr(words),
                                      ptr(vals), ptr(common), ptr(score), 0) == OK
    np.testing.assert_array_equal(common, want_c)
    np.testing.assert_array_equal(score.view(np.uint32), want_s.view(np.uint32))
    # the device entry point on torch tensors, with the offsets as they are (kf_off[0] = lead)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a) if len(a) else np.zeros(1, a.dtype)).to(gpu)
    tq, tv, to, tw, tx = t(qw.view(np.int32)), t(qv), t(off), t(words.view(np.int32)), t(vals)
    tc = torch.full((nkf,), -7, dtype=torch.int32, device=gpu)
    ts = torch.full((nkf,), -7, dtype=torch.float32, device=gpu)
    torch.cuda.synchronize()
    assert orbx_lib.orbx_bow_db_score_device(ptr(tq), ptr(tv), len(qw), nkf, ptr(to), ptr(tw),
                                             ptr(tx), ptr(tc), ptr(ts), None) == OK
    torch.cuda.synchronize()
    np.testing.assert_array_equal(tc.cpu().numpy(), want_c)
    np.testing.assert_array_equal(ts.cpu().numpy().view(np.uint32), want_s.view(np.uint32))


@pytest.mark.gpu
def test_gpu_bow_db_score_query_limit(oracle_mod, orbx_lib, gpu):
    from my_orb_slam2_amd.vocabulary import bow_db_score, bow_db_score_max_query
    from my_orb_slam2_amd._lib import OrbxError
    m = bow_db_score_max_query()
    rng = np.random.default_rng(16)
    q = (np.arange(m + 1, dtype=np.uint32) * 3, rng.random(m + 1) / m)
    kfs = [(q[0][::7].copy(), rng.random(len(q[0][::7]))), (q[0][m - 1:m].copy(), np.array([0.5])),
           (q[0][m:].copy(), np.array([0.5]))]
    qm = (q[0][:m], q[1][:m])
    common, score = bow_db_score(qm, kfs)
    want_c, want_s = _expected_scores(qm, kfs)
    assert list(want_c[1:]) == [1, 0]       # the last admitted word is seen, the next is not
    np.testing.assert_array_equal(common, want_c)
    np.testing.assert_array_equal(score.view(np.uint32), want_s.view(np.uint32))
    with pytest.raises(OrbxError) as e:
        bow_db_score(q, kfs)
    assert e.value.code == ERR_UNSUPPORTED


@pytest.mark.gpu
def test_gpu_bow_db_score_sentinels(oracle_mod, orbx_lib, gpu):
    """orbx_bow_db_score with two keyframes, three query words and kf_off[0] = 5, the outputs
    inside sentinel-filled allocations: nkf values each, the restatement's; nothing else written."""
    import host_array_cases as hc
    c = hc.case("bow_db_score")
    r = c.call()
    assert r["common"].guards_intact() and r["score"].guards_intact()
    want_c, want_s = _expected_scores(c.q, c.kfs)
    assert want_c.tolist() == [2, 1]
    np.testing.assert_array_equal(r["common"].a, want_c)
    np.testing.assert_array_equal(r["score"].a.view(np.uint32), want_s.view(np.uint32))
