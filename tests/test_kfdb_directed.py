"""Directed KeyFrameDatabase cases on the CPU (tests/kfdb_cases.py): the C++ oracle against the
pure-Python restatement on every case (candidate lists and every read-back array, floats as
bits), the stated expectations, and the census: every construct name occurs and every
`variant=` of the restatement changes the result of at least one case, so a case set that
stopped distinguishing a decision fails here and not silently on the GPU."""
import numpy as np
import pytest

import kfdb_cases as kc
from kfdb_cases import CASES, PyKeyFrameDatabase

IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def restated():
    """The restatement's (candidates, record) per query of every case, computed once."""
    return {c["name"]: kc.run_case(PyKeyFrameDatabase(c["K"], record=True), c, kc.read_py)
            for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_equals_restatement(oracle_mod, restated, case):
    from oracle.kfdb import OracleKeyFrameDatabase
    got = kc.run_case(OracleKeyFrameDatabase(case["K"]), case, lambda d: d.debug_read())
    want = restated[case["name"]]
    assert len(got) == len(want) > 0
    for q, ((oc, orb), (pc, prb)) in enumerate(zip(got, want)):
        where = f"{case['name']} query {q}"
        assert oc == pc, where
        kc.assert_oracle_record(prb, orb, where)


@pytest.mark.parametrize("case", [c for c in CASES if c["expect"] is not None],
                         ids=[c["name"] for c in CASES if c["expect"] is not None])
def test_stated_expectations(restated, case):
    assert [c for c, _ in restated[case["name"]]] == case["expect"]


def test_planted_values(restated):
    """What the docstrings of the cases claim about accumulated scores and best keyframes."""
    r = {k: v for k, v in restated.items()}
    acc = r["acc_float32"][0][1]["acc"]
    assert acc[0] == np.float32(0.5)                       # 0.5 + 2^-25 + 2^-25 in float32
    t = r["best_ties"][0][1]
    assert list(t["best"]) == [0, 1, 3, 3] and t["acc"][1] == 1.0 and t["acc"][2] == 1.0
    for K in (1, 10, 64):
        for tag in ("exactly", "over"):
            for _, rec in r[f"row_{tag}_K{K}"]:
                assert rec["acc"][0] == np.float32(0.5 + K / 64.0), (K, tag)
    for name, q in (("reloc_nb_stored", 1), ("state_query_before_last", 2),
                    ("state_survives_growth", 1)):
        assert r[name][q][1]["acc"][0] == np.float32(0.75), name       # 0.5 + stored 0.25
    for name, q in (("state_zero_initially", 0), ("state_zero_after_clear", 1)):
        assert r[name][q][1]["acc"][0] == np.float32(0.5), name
    assert r["loop_exclusion"][0][1]["acc"][1] == np.float32(0.25)
    assert r["loop_nb_below_minc"][0][1]["acc"][0] == np.float32(0.25)
    e = r["erased"][0][1]
    assert e["best"][0] == 2 and e["acc"][0] == np.float32(1.25) and e["common"][1] == 0
    s = r["scan_order_dependent_sum"][0][1]["score"]
    assert s[0] == np.float32(2.0**52)
    assert r["scan_float32_sum"][0][1]["score"][0] == np.float32(0.5 + 2.0**-24)
    sz = r["scan_sizes"][0][1]
    assert list(sz["common"]) == [0, 1, 63, 64, 65, 128, 129]
    ch = r["scan_chunks"][0][1]
    assert list(ch["first"]) == [3, 5, 1, 2] and list(ch["common"]) == [1, 2, 1, 1]
    z = r["all_scores_zero"]
    assert z[0][1]["selected"] and np.all(z[0][1]["best"] >= 0) and z[0][0] == []


def test_census_constructs():
    planted = [x for c in CASES for x in c["constructs"]]
    assert sorted(set(planted)) == sorted(kc.CONSTRUCTS)


@pytest.mark.parametrize("variant", kc.VARIANTS)
def test_census_variant_changes_a_case(restated, variant):
    changed = []
    for c in CASES:
        if len(c["steps"]) > 400:   # the large databases repeat what small cases decide
            continue
        got = kc.run_case(PyKeyFrameDatabase(c["K"], variant=variant), c, kc.read_py)
        want = restated[c["name"]]
        if any(gc != wc or not kc.same_record(gr, wr) for (gc, gr), (wc, wr) in zip(got, want)):
            changed.append(c["name"])
    assert changed, f"no case tells `{variant}` from the reference"


def test_filter_float_remark():
    """int(mx * 0.8f) in float32 equals int(mx * 0.8) in double for every mx <= 8192."""
    mx = np.arange(1, 8193)
    f = (mx.astype(np.float32) * np.float32(0.8)).astype(np.int64)
    d = (mx.astype(np.float64) * 0.8).astype(np.int64)
    g = (mx.astype(np.float64) * float(np.float32(0.8))).astype(np.int64)
    assert np.array_equal(f, d) and np.array_equal(f, g)
