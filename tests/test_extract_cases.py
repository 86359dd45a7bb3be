"""CPU: the directed extractor cases (tests/extract_cases.py) do what they say.

1. Prediction: on every single-level case the oracle's level-0 FAST candidates equal the
   closed-form prediction from the stamps (positions, responses, order), and the outcome
   written beside every planted construct holds.
2. Octree: octree_reference over the candidates equals the oracle's level keypoints on every
   level of every case, and reports the events of the run.
3. Orientation: the integer moments over the umax circle, through fast_atan2, equal the
   oracle's angles; planted (m10, m01) values occur; a ballast pixel one past the circle
   changes no angle.
4. Census: every construct name is backed by a check that reads the run (not the label),
   every octree event occurs, and every ``variant=`` (one flipped decision each) changes the
   result of at least one case.
"""
import types

import numpy as np
import pytest

import extract_cases as ec

NAMES = [c.name for c in ec.cases()]
SINGLE = [c.name for c in ec.cases() if c.single_level]
CASE = {c.name: c for c in ec.cases()}

_RUNS = {}


def _kp3(k, off=0):
    return [(int(q["x"]) - off, int(q["y"]) - off, float(q["response"])) for q in k]


def run_of(oracle_mod, name):
    """The oracle's run of a case, its prediction and its octree events (computed once)."""
    if name not in _RUNS:
        c = CASE[name]
        o = oracle_mod.OracleExtractor(*c.params)
        kps, desc = o(c.img)
        r = types.SimpleNamespace(case=c, o=o, kps=kps, desc=desc, ev=[], pred=None, cells=None)
        nl = c.params[2]
        quotas = o.tables()["features_per_level"]
        r.cands = [[(x, y, s) for x, y, s in _kp3(o.candidates(l))] for l in range(nl)]
        r.level_kps = [o.level_keypoints(l) for l in range(nl)]
        r.oct = []
        for l in range(nl):
            w, h = o.level_size(l)
            ev = {}
            r.oct.append(ec.octree_reference(r.cands[l], 16, w - 16, 16, h - 16, int(quotas[l]),
                                             events=ev))
            r.ev.append(ev)
        if c.single_level:
            r.pred, r.cells = c.prediction()
        _RUNS[name] = r
    return _RUNS[name]


# ---- the builder's own invariants ------------------------------------------------------------
def test_builder_rejects_what_breaks_the_argument():
    with pytest.raises(AssertionError, match="closer than 4"):
        ec.StampImage(96, 80).dot(30, 30, 50).dot(33, 30, 50).check()
    with pytest.raises(AssertionError, match="closer than 4"):
        ec.StampImage(96, 80).dot(30, 30, 50).ballast(32, 33, 5).check()
    ec.StampImage(96, 80).dot(30, 30, 50).dot(34, 30, 50).ballast(30, 34, 7).check()
    with pytest.raises(AssertionError, match="above minThFAST"):
        ec.StampImage(96, 80).ballast(30, 30, 8)
    with pytest.raises(AssertionError, match="outside"):
        ec.StampImage(96, 80).pair(95, 30, 50, 50, "h")
    with pytest.raises(AssertionError):
        ec.dot_field(96, 80, 3, 0, 10)


def test_pitch_3_breaks_the_prediction(oracle_mod):
    """Why the spacing is 4: at pitch 3 a dot lies on its neighbours' circles and the oracle
    finds fewer keypoints than one per dot."""
    rng = np.random.default_rng(0)
    img = np.zeros((80, 96), np.uint8)
    n = 0
    for y in range(19, 60, 3):
        for x in range(19, 76, 3):
            img[y, x] = rng.integers(21, 120)
            n += 1
    o = oracle_mod.OracleExtractor(5000, 1.2, 1, 20, 7)
    o(img)
    assert len(o.candidates(0)) < n


# ---- 1. prediction ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", SINGLE)
def test_prediction_equals_oracle(oracle_mod, name):
    r = run_of(oracle_mod, name)
    assert r.cands[0] == [(x, y, s) for x, y, s, _, _ in r.pred]


@pytest.mark.parametrize("name", [n for n in SINGLE if CASE[n].expect])
def test_planted_outcomes(oracle_mod, name):
    r = run_of(oracle_mod, name)
    c = r.case
    by_pos = {(x, y): (s, p) for x, y, s, _, p in r.pred}
    final = _kp3(r.level_kps[0], 16)
    for construct, kind, data in c.expect:
        what = f"{name}: {construct}"
        if kind == "fast":
            assert data, what
            for x, y, s, p in data:
                assert by_pos.get((x, y)) == (float(s), p), (what, (x, y, s, p), by_pos.get((x, y)))
        elif kind == "nofast":
            assert data, what
            for x, y in data:
                assert (x, y) not in by_pos, (what, (x, y))
                assert (x + 16, y + 16) in c.st.corners, (what, "not a planted pixel")
        elif kind == "cell_corners":
            cell, n = data
            assert r.cells[cell]["corners"][0] == n, (what, r.cells[cell])
        elif kind == "octree":
            assert final == [(x, y, float(s)) for x, y, s in data], (what, final)
        elif kind == "octree_roots":
            w = c.img.shape[1]
            hx = np.float32(w - 32) / np.float32(r.ev[0]["roots"])
            xs = sorted({x for x, _, _ in r.cands[0]})
            assert any(int(np.float32(a) / hx) + 1 == int(np.float32(a + 1) / hx) and a + 1 in xs
                       for a in xs), what
            assert float(hx) != int(hx), what
        elif kind == "octree_roots_dropped":
            assert r.ev[0]["roots_dropped"] == data, what
            roots = sorted({int(np.float32(x) / (np.float32(c.img.shape[1] - 32) /
                                                np.float32(r.ev[0]["roots"])))
                            for x, _, _ in r.cands[0]})
            assert roots == [0, 2], (what, roots)
        elif kind == "count":
            assert len(r.kps) == data, what
        elif kind in ("moments", "twins"):
            pass    # test_orientation_*
        else:
            raise AssertionError(f"unknown expectation kind {kind}")


def test_floors(oracle_mod):
    """The oracle's keypoint counts recorded in the table (the GPU tests assert them before
    they compare anything)."""
    got = {n: len(run_of(oracle_mod, n).kps) for n in NAMES}
    assert got == ec.FLOORS


# ---- 2. octree -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_octree_restatement_equals_oracle(oracle_mod, name):
    r = run_of(oracle_mod, name)
    for l, lk in enumerate(r.level_kps):
        assert _kp3(lk, 16) == r.oct[l], f"{name} level {l}"


# ---- 3. orientation --------------------------------------------------------------------------
def _angles(oracle_mod, r, stride=1):
    """[(level, x, y, m10, m01)] of every stride-th keypoint of a run, each checked against
    the oracle's angle."""
    out = []
    for l, lk in enumerate(r.level_kps):
        img = r.o.level(l)
        for k in lk[::stride]:
            x, y = int(k["x"]), int(k["y"])
            m10, m01 = ec.moments(img, x, y)
            ang = np.float32(oracle_mod.fast_atan2(float(m01), float(m10)))
            assert ang == k["angle"], (r.case.name, l, x, y, m10, m01)
            out.append((l, x, y, m10, m01))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_orientation_restatement_equals_oracle(oracle_mod, name):
    r = run_of(oracle_mod, name)
    got = _angles(oracle_mod, r, 1 if len(r.kps) <= 200 else 9)
    assert len(got) >= min(len(r.kps), 1)


def test_planted_moments(oracle_mod):
    r = run_of(oracle_mod, "moments_exact")
    (_, _, moms), = [e for e in r.case.expect if e[1] == "moments"]
    got = {(x - 16, y - 16): (m10, m01) for _, x, y, m10, m01 in _angles(oracle_mod, r)}
    ang = {(int(k["x"]) - 16, int(k["y"]) - 16): float(k["angle"]) for k in r.kps}
    for name, (pos, m) in moms.items():
        assert got[pos] == m, name
    A = lambda n: ang[moms[n][0]]
    assert moms["zero"][1] == (0, 0) and moms["cancel"][1] == (0, 0)
    assert A("zero") == A("cancel") == float(np.float32(oracle_mod.fast_atan2(0.0, 0.0)))
    for n, deg in (("axis_0", 0), ("axis_90", 90), ("axis_180", 180), ("axis_270", 270),
                   ("diag_45", 45), ("diag_135", 135), ("diag_225", 225), ("diag_315", 315)):
        # fastAtan2 is a polynomial: exact on the axes, within its published 0.3 degrees elsewhere
        assert abs(A(n) - deg) <= (0.0 if deg % 90 == 0 else 0.3), (n, A(n))
    assert moms["huge_tiny"][1] == (15 * 60 + 14 * 120 + 13 * 60, 4)
    assert moms["tiny_huge"][1] == (-4, 15 * 60 + 14 * 120 + 13 * 60)


@pytest.mark.parametrize("name", ["umax_circle_pos", "umax_circle_neg"])
def test_pixel_past_the_circle_changes_no_angle(oracle_mod, name):
    r = run_of(oracle_mod, name)
    (_, _, twins), = [e for e in r.case.expect if e[1] == "twins"]
    ang = {(int(k["x"]) - 16, int(k["y"]) - 16): k["angle"] for k in r.kps}
    img = r.case.img.astype(int)
    s = 1 if name.endswith("pos") else -1
    for v in range(16):
        a, b = twins[2 * v], twins[2 * v + 1]
        d = ec.UMAX[v]
        # the inside pixel is there and counts; the twin's extra pixel is there (but for
        # |v| <= 3, where it would fall outside the 31 x 31 patch) and does not
        for (x, y) in (a, b):
            assert img[y + 16 + s * v, x + 16 + s * d] == 50
        if d + 1 <= 15:
            assert img[b[1] + 16 + s * v, b[0] + 16 + s * (d + 1)] == 60
        assert ang[a] == ang[b], (v, ang[a], ang[b])
        base = np.float32(oracle_mod.fast_atan2(float(-6 * s * 31), float(-4 * s * 31)))
        assert ang[a] != base, v
    # one umax entry one too wide changes at least one twin's moments
    for v in range(4, 16):
        wide = list(ec.UMAX)
        wide[v] += 1
        x, y = twins[2 * v + 1]
        assert ec.moments(img, x + 16, y + 16, wide) != ec.moments(img, x + 16, y + 16), v


# ---- 4. census -------------------------------------------------------------------------------
def _cells_with_content(r):
    g = ec.cell_grid(r.case.img.shape[1], r.case.img.shape[0])
    return [c for c, info in zip(g["cells"], r.cells) if info["n"] > 0]


def _ev0(f):
    return lambda r: f(r.ev[0])


def _planted(name):
    return lambda r: any(e[0] == name for e in r.case.expect)   # test_planted_outcomes checks it


def _nt_cut(n, past=0):
    return _ev0(lambda e: any(c[0] == n + past and c[1] > n + past for c in e["cuts"]))


CHECKS = {
    # FAST: outcome lists beside the stamps
    **{n: _planted(n) for n in (
        "fallback_cell", "ini_among_sub_ini", "tied_pairs_empty_ini", "pair_larger_wins",
        "pair_ini_and_sub_ini", "sub_ini_pairs", "pair_across_cells", "extreme_score_254",
        "position_edges", "ini_keypoint_is_corner_65_plus", "cell_of_64_corners",
        "cell_of_65_corners", "fallback_after_65_corners", "root_last_first_column",
        "empty_root_between", "node_of_one_key", "ini_equals_min")},
    "threshold_edges": lambda r: {r.case.params[3], r.case.params[3] + 1, r.case.params[4],
                                  r.case.params[4] + 1} <= set(r.case.st.corners.values()),
    "polarity_bright": lambda r: r.case.st.bg == 0 and len(r.kps) > 0,
    "polarity_dark": lambda r: r.case.st.bg == 255 and len(r.kps) > 0,
    # cell geometry, with content in the cells meant
    "rows_gt_40": lambda r: any(c[5] - c[3] > 40 for c in _cells_with_content(r)),
    "rows_le_40": lambda r: any(c[5] - c[3] <= 40 for c in _cells_with_content(r)),
    "dw_gt_32": lambda r: any(c[4] - c[2] - 6 > 32 for c in _cells_with_content(r)),
    "dw_le_32": lambda r: any(c[4] - c[2] - 6 <= 32 for c in _cells_with_content(r)),
    "ini_x_residues": lambda r: {c[2] & 3 for c in _cells_with_content(r)} == {0, 1, 2, 3},
    # octree: from the events of the run
    "n_ini_1": _ev0(lambda e: e["roots"] == 1),
    "n_ini_2": _ev0(lambda e: e["roots"] == 2),
    "n_ini_3": _ev0(lambda e: e["roots"] >= 3),
    "best_tie_cell_major": lambda r: r.case.octree(r.pred) != r.case.octree(
        r.case.prediction("raster_order")[0]),
    "best_tie_in_cell": _ev0(lambda e: e["best_ties"] >= 2),
    "quota_1": lambda r: r.case.params[0] == 1 and len(r.kps) > 0,
    "quota_0": lambda r: r.case.params[0] == 0 and len(r.kps) > 0,
    "end_S_gt_N": _ev0(lambda e: e["end"] == "S>N"),
    "end_S_eq_N": _ev0(lambda e: e["end"] == "S==N" and e["rounds2"] > 0),
    "end_S_eq_N_phase1": _ev0(lambda e: e["end"] == "S==N" and e["rounds2"] == 0),
    "end_S_eq_prevS": _ev0(lambda e: e["end"] == "S==prevS"),
    "N_above_candidates": lambda r: r.case.params[0] > len(r.cands[0]) > 0,
    "phase2_switch": _ev0(lambda e: e["rounds2"] > 0),
    "small_list": _ev0(lambda e: 0 < e["max_list"] < 512),
    "keys_on_split_x": _ev0(lambda e: e["on_split_x"] > 0),
    "keys_on_split_y": _ev0(lambda e: e["on_split_y"] > 0),
    "keys_on_odd_split": _ev0(lambda e: e["on_split_odd"] >= 3 and e["odd_splits"] > 0),
    "one_quadrant_rounds": lambda r: r.ev[0]["one_quadrant_rounds"] >= 2 and
    len(r.kps) == len(r.cands[0]),
    "stop_while_expandable": lambda r: r.ev[0]["end"] == "S==prevS" and
    len(r.kps) < len(r.cands[0]) < r.case.params[0],
    "cut_at_128": _nt_cut(128), "cut_past_128": _nt_cut(128, 1),
    "cut_at_256": _nt_cut(256), "cut_past_256": _nt_cut(256, 1),
    "expandable_above_nt": _ev0(lambda e: e["rounds2"] > 0 and e["max_expandable"] > 256),
    # ncap = align16(nfeatures + 3) against the 256 threads of a single frame's list
    "bucket_sort": lambda r: r.ev[0]["rounds2"] > 0 and r.case.params[0] + 3 >= 256,
    "rank_sort_ncap_lt_nt": lambda r: r.ev[0]["rounds2"] > 0 and r.case.params[0] + 3 + 15 < 256,
    "seq_ties": _ev0(lambda e: e["seq_ties"] > 0),
    "seq_tie_at_cut": _ev0(lambda e: e["seq_ties_at_cut"] > 0),
    "switch_margin_0": _ev0(lambda e: any(s + 3 * n == 128 for s, n in e["phase1"][:-1])
                            and e["switch_margin"] != 0),
    "switch_margin_1": _ev0(lambda e: e["switch_margin"] == 1),
    "big_nodes_distinct": _ev0(lambda e: e["big_distinct"] > 0),
    "big_nodes_equal": _ev0(lambda e: e["big_equal"] > 0),
    "list_crosses_512_phase1": _ev0(lambda e: any(s >= 512 for s, _ in e["phase1"][:-1])
                                    and e["rounds2"] == 0),
    # orientation
    "m10_m01_zero": _planted("planted_moments"), "axis_angles": _planted("planted_moments"),
    "diagonal_angles": _planted("planted_moments"), "huge_beside_tiny": _planted("planted_moments"),
    "umax_edge": _planted("umax_edge"),
    "x_mod_16_y_mod_4": lambda r: len({int(k["x"]) % 16 for k in r.kps}) >= 8 and
    {int(k["y"]) % 4 for k in r.kps} == {0, 1, 2, 3},
    "x_mod_16_all": lambda r: {int(k["x"]) % 16 for k in r.kps} == set(range(16)) and
    {int(k["y"]) % 4 for k in r.kps} == {0, 1, 2, 3},
    "extreme_coordinates": lambda r: {(int(k["x"]), int(k["y"])) for k in r.kps} >= {
        (19, 19), (r.case.img.shape[1] - 20, 19), (19, r.case.img.shape[0] - 20),
        (r.case.img.shape[1] - 20, r.case.img.shape[0] - 20)},
    **{f"level_count_{n}": (lambda n: lambda r: len(r.kps) == n)(n)
       for n in (1, 2, 7, 8, 9, 31, 32, 33)},
    # multi-level: keypoints on more than one level, the last one included for 3
    "nlevels_3": lambda r: r.case.params[2] == 3 and all(len(k) > 0 for k in r.level_kps),
    "nlevels_8": lambda r: r.case.params[2] == 8 and sum(len(k) > 0 for k in r.level_kps) >= 3,
    "thresholds_out_of_range": lambda r: r.case.params[3] > 255 and r.case.params[4] < 0 and
    len(r.kps) > 0,
    "quota_0_level": lambda r: int(r.o.tables()["features_per_level"][-1]) == 0 and
    len(r.level_kps[-1]) > 0,
    "textured": lambda r: r.case.st is None and len(r.kps) >= 200,
}
CHECKS["score_0_never_survives"] = _planted("score_0_never_survives")


def test_census_constructs(oracle_mod):
    """Every construct a case lists is backed by its check on that case's run, and every
    check is listed by some case (deleting a case leaves a construct without one, or the case
    was redundant)."""
    seen = set()
    for name in NAMES:
        r = run_of(oracle_mod, name)
        for con in r.case.constructs:
            assert con in CHECKS, f"{name}: construct {con} has no check"
            assert CHECKS[con](r), f"{name}: construct {con} does not occur"
            seen.add(con)
    assert seen >= set(CHECKS) - {"score_0_never_survives"}, sorted(set(CHECKS) - seen)
    assert CHECKS["score_0_never_survives"](run_of(oracle_mod, "thresholds_0_0"))
    # every case is the only holder of at least one construct, or one of a parametrised family
    holders = {}
    for c in ec.cases():
        for con in c.constructs:
            holders.setdefault(con, []).append(c.name)
    for c in ec.cases():
        assert any(len(holders[con]) == 1 for con in c.constructs) or \
            c.name.startswith(("thresholds_", "extremes_", "umax_circle_")) or \
            c.name.endswith(("_L3", "_L8")), f"{c.name} is redundant: {c.constructs}"


def test_census_events(oracle_mod):
    hit = set()
    for name in NAMES:
        for ev in run_of(oracle_mod, name).ev:
            hit |= {k for k in ec.OCTREE_EVENTS if ev.get(k)}
    assert hit == set(ec.OCTREE_EVENTS), sorted(set(ec.OCTREE_EVENTS) - hit)


def test_census_variants(oracle_mod):
    """Each variant flips one decision of the restatement; each must change the final level-0
    keypoints of at least one single-level case (so a kernel that took the flipped decision
    would differ from the oracle on that case).  Prints which."""
    hits = {}
    for name in SINGLE:
        r = run_of(oracle_mod, name)
        c = r.case
        base = c.octree(r.pred)
        assert [k[:3] for k in base] == r.oct[0]
        for v in ec.FAST_VARIANTS:
            if c.octree(c.prediction(v)[0]) != base:
                hits.setdefault(v, []).append(name)
        for v in ec.OCTREE_VARIANTS:
            if c.octree(r.pred, v) != base:
                hits.setdefault(v, []).append(name)
    for v in ec.FAST_VARIANTS + ec.OCTREE_VARIANTS:
        print(f"variant {v}: {hits.get(v, [])}")
    missing = [v for v in ec.FAST_VARIANTS + ec.OCTREE_VARIANTS if v not in hits]
    assert not missing, missing
