"""Directed KeyFrameDatabase cases on the GPU (tests/kfdb_cases.py): the HBM-resident database
(csrc/orbx_kfdb.hip) equals the C++ oracle on every case: candidate lists in order, and per
slot the scan's common / first, the selection's best as integers and score / acc / state bit
for bit (orbx_kfdb_debug_read against the oracle's read-back and the restatement's record).
Then the limits of orbx_kfdb_limits with their status codes, and the library-defined
behaviour for a covisible entry >= nslots.  Everything is exact."""
import ctypes

import numpy as np
import pytest

import kfdb_cases as kc
from kfdb_cases import CASES, PyKeyFrameDatabase

pytestmark = pytest.mark.gpu

OK, ERR_INVALID, ERR_CAPACITY, ERR_UNSUPPORTED, ERR_STATE = 0, -1, -3, -4, -5


def assert_gpu_record(py, g, where=""):
    """orbx_kfdb_debug_read against the restatement's record (all slots, floats as bits)."""
    np.testing.assert_array_equal(g["common"], py["common"], where)
    np.testing.assert_array_equal(g["first"], py["first"], where)
    np.testing.assert_array_equal(kc.bits(g["score"]), kc.bits(py["score"]), where)
    np.testing.assert_array_equal(kc.bits(g["state"]), kc.bits(py["state"]), where)
    if py["selected"]:   # the selection returns before it writes these when no slot is listed
        np.testing.assert_array_equal(g["best"], py["best"], where)
        np.testing.assert_array_equal(kc.bits(g["acc"]), kc.bits(py["acc"]), where)


def assert_gpu_oracle(g, o, connected, where=""):
    """orbx_kfdb_debug_read against the oracle's read-back, where the oracle defines it: words
    and first of the keyframes it listed, 0 / INT_MAX of unconnected ones it did not."""
    n = len(g["common"])
    listed = o["listed"][:n].astype(bool)
    conn = np.array([s in connected for s in range(n)], bool)
    np.testing.assert_array_equal(g["common"][listed], o["words"][:n][listed], where)
    np.testing.assert_array_equal(g["first"][listed], o["first"][:n][listed], where)
    assert np.all(g["common"][~listed & ~conn] == 0), where
    assert np.all(g["first"][~listed & ~conn] == kc.INT_MAX), where
    np.testing.assert_array_equal(kc.bits(g["score"]), kc.bits(o["score"][:n]), where)
    np.testing.assert_array_equal(kc.bits(g["state"]), kc.bits(o["reloc_score"][:n]), where)
    if o["selected"]:
        np.testing.assert_array_equal(g["best"], o["best"][:n], where)
        np.testing.assert_array_equal(kc.bits(g["acc"]), kc.bits(o["acc"][:n]), where)


@pytest.fixture(scope="module")
def reference(oracle_mod):
    """(candidates, oracle read-back, restatement record) per query of every case, once."""
    from oracle.kfdb import OracleKeyFrameDatabase
    ref = {}
    for c in CASES:
        o = kc.run_case(OracleKeyFrameDatabase(c["K"]), c, lambda d: d.debug_read())
        p = kc.run_case(PyKeyFrameDatabase(c["K"], record=True), c, kc.read_py)
        assert [x for x, _ in o] == [x for x, _ in p], c["name"]
        ref[c["name"]] = [(oc, orb, prb) for (oc, orb), (_, prb) in zip(o, p)]
    return ref


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_gpu_equals_oracle(orbx_lib, gpu, reference, case):
    from my_orb_slam2_amd import KeyFrameDatabase
    g = KeyFrameDatabase(case["K"])
    got = kc.run_case(g, case, lambda d: d.debug_read())
    g.close()
    want = reference[case["name"]]
    assert len(got) == len(want) > 0
    for q, ((gc, grb), (oc, orb, prb)) in enumerate(zip(got, want)):
        where = f"{case['name']} query {q}"
        print(where, "candidates", gc, "best", grb["best"][:8])
        assert gc == oc, where
        assert_gpu_oracle(grb, orb, prb["connected"], where)
        assert_gpu_record(prb, grb, where)


def _both(K=10):
    from my_orb_slam2_amd import KeyFrameDatabase
    from oracle.kfdb import OracleKeyFrameDatabase
    return KeyFrameDatabase(K), OracleKeyFrameDatabase(K)


def test_limit_query_words(orbx_lib, gpu, oracle_mod):
    """nq = QMAX runs (the scan's dynamic LDS needs the raised attribute); QMAX + 1 does not."""
    from my_orb_slam2_amd import KeyFrameDatabase
    lim = KeyFrameDatabase.limits()
    g, o = _both()
    for d in (g, o):
        d.add(kc.kf([lim["QMAX"] - 1], 0.75))   # the query's last word
        d.add(kc.kf([0], 0.75))                 # its first: listed before slot 0
        d.add(kc.kf([lim["QMAX"]], 1.0))        # one past the query
    q = kc.query(range(lim["QMAX"]))
    code, n, cand = g.detect_raw(q)
    assert code == OK and list(cand) == list(o.DetectRelocalizationCandidates(q)) == [1, 0]
    rb = g.debug_read()
    assert list(rb["first"]) == [lim["QMAX"] - 1, 0, kc.INT_MAX] and list(rb["common"]) == [1, 1, 0]
    code, n, cand = g.detect_raw(q, connected=[], min_score=0.0)
    assert code == OK and list(cand) == list(o.DetectLoopCandidates(q, [], 0.0))
    q1 = kc.query(range(lim["QMAX"] + 1))
    assert g.detect_raw(q1)[0] == ERR_UNSUPPORTED
    assert g.detect_raw(q1, connected=[], min_score=0.0)[0] == ERR_UNSUPPORTED
    g.close()


def test_limit_connected(orbx_lib, gpu, oracle_mod):
    from my_orb_slam2_amd import KeyFrameDatabase
    lim = KeyFrameDatabase.limits()
    g, o = _both()
    for d in (g, o):
        for s in range(4):
            d.add(kc.kf([10], (s + 1) / 8.0))
    # slot 3 (the best score) and slot 1 connected, the rest of the list beyond the database
    conn = [3, 1] + list(range(100, 100 + lim["EXCL_MAX"] - 2))
    assert len(conn) == lim["EXCL_MAX"]
    code, n, cand = g.detect_raw(kc.Q1, connected=conn, min_score=0.0)
    assert code == OK and list(cand) == list(o.DetectLoopCandidates(kc.Q1, conn, 0.0)) == [2]
    assert g.detect_raw(kc.Q1, connected=conn + [7], min_score=0.0)[0] == ERR_UNSUPPORTED
    g.close()


def test_limit_retained_and_capacity(orbx_lib, gpu, oracle_mod):
    """RCAP identical one-word keyframes are all retained and come back in slot order (the
    full-width bitonic sort); one more is ORBX_ERR_UNSUPPORTED.  A `cap` one below the count
    gives ORBX_ERR_CAPACITY with the true count and the first `cap` entries."""
    from my_orb_slam2_amd import KeyFrameDatabase
    rcap = KeyFrameDatabase.limits()["RCAP"]
    g, o = _both()
    b = kc.kf([10], 0.5)
    for _ in range(rcap):
        g.add(b)
        o.add(b)
    code, n, cand = g.detect_raw(kc.Q1)
    assert code == OK and n == rcap
    assert np.array_equal(cand, np.arange(rcap))
    assert np.array_equal(o.DetectRelocalizationCandidates(kc.Q1), np.arange(rcap))
    code, n, cand = g.detect_raw(kc.Q1, cap=rcap - 1)
    assert code == ERR_CAPACITY and n == rcap and np.array_equal(cand, np.arange(rcap - 1))
    code, n, cand = g.detect_raw(kc.Q1, connected=[5], min_score=0.5, cap=rcap - 2)
    assert code == ERR_CAPACITY and n == rcap - 1
    assert np.array_equal(cand, np.delete(np.arange(rcap), 5)[:rcap - 2])
    g.add(b)
    assert g.detect_raw(kc.Q1)[0] == ERR_UNSUPPORTED
    # with one of them connected the loop query retains RCAP again
    code, n, cand = g.detect_raw(kc.Q1, connected=[0], min_score=0.0)
    assert code == OK and np.array_equal(cand, np.arange(1, rcap + 1))
    g.close()


def test_capacity_small(orbx_lib, gpu):
    from my_orb_slam2_amd import KeyFrameDatabase
    case = next(c for c in CASES if c["name"] == "list_order")
    g = KeyFrameDatabase(10)
    for st in case["steps"]:
        if st[0] == "add":
            g.add(st[1])
    for cap in (2, 1, 0):
        code, n, cand = g.detect_raw(kc.Q5, cap=cap)
        assert code == ERR_CAPACITY and n == 3 and list(cand) == [1, 2, 0][:cap]
    code, n, cand = g.detect_raw(kc.Q5, cap=3)
    assert code == OK and list(cand) == [1, 2, 0]
    g.close()


def test_covisible_beyond_database_is_skipped(orbx_lib, gpu):
    """Library-defined (the reference would index past its keyframes): an entry >= nslots in
    a covisibility row changes nothing, entries after it still count."""
    from my_orb_slam2_amd import KeyFrameDatabase
    out = []
    for row in ([1], [3, 1], [1000000, 1, 2**31 - 1]):
        g = KeyFrameDatabase(10)
        g.add(kc.kf([10], 0.5))
        g.add(kc.kf([10], 0.75))
        g.add(kc.kf([11], 0.25))
        g.set_covisibles(0, row)
        res = []
        for loop in (False, True):
            c = g.DetectLoopCandidates(kc.Q1, [], 0.0) if loop else \
                g.DetectRelocalizationCandidates(kc.Q1)
            rb = g.debug_read()
            res.append((list(c), list(rb["best"]), list(kc.bits(rb["acc"]))))
        out.append(res)
        g.close()
    assert out[0][0] == ([1], [1, 1, -1], list(kc.bits([1.25, 0.75, -1.0])))
    assert out[1] == out[0] and out[2] == out[0]


def test_limit_covisibles(orbx_lib, gpu):
    from my_orb_slam2_amd import KeyFrameDatabase
    from my_orb_slam2_amd._lib import OrbxError
    kmax = KeyFrameDatabase.limits()["KMAX"]
    KeyFrameDatabase(kmax).close()
    for k in (kmax + 1, 0):
        with pytest.raises(OrbxError) as e:
            KeyFrameDatabase(k)
        assert e.value.code == ERR_INVALID


def test_debug_read_contract(orbx_lib, gpu):
    from my_orb_slam2_amd import KeyFrameDatabase
    L = orbx_lib
    g = KeyFrameDatabase(10)
    g.add(kc.kf([10], 0.5))
    g.add(kc.kf([10], 0.25))
    one = np.zeros(2, np.int32)
    none = ctypes.c_void_p(0)
    args = lambda n, best: (g._h, none, none, none, none, none, best, n)
    assert L.orbx_kfdb_debug_read(*args(2, one.ctypes.data)) == ERR_STATE   # nothing uploaded
    assert L.orbx_kfdb_debug_read(*args(3, one.ctypes.data)) == ERR_INVALID
    assert L.orbx_kfdb_debug_read(*args(0, none)) == OK
    assert list(g.DetectRelocalizationCandidates(kc.Q1)) == [0]
    assert L.orbx_kfdb_debug_read(*args(2, one.ctypes.data)) == OK and list(one) == [0, 1]
    assert L.orbx_kfdb_debug_read(*args(2, none)) == OK                      # all outputs NULL
    g.close()
