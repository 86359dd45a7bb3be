"""CPU: the directed cases of tests/frame_cases.py for the per-frame geometry kernels (k_undistort,
k_grid, k_gray, k_frustum).  The plain restatements against the C++ oracle on every case (and
against features.assign_features_to_grid on the default grid); the census of what the cases
contain, asserted on the restatement alone; every single-decision variant of a restatement changes
a directed case; the argument refusals of the grid entry points, which need no GPU."""
import ctypes

import numpy as np
import pytest

import frame_cases as fc
from my_orb_slam2_amd.features import assign_features_to_grid

f32 = np.float32


@pytest.fixture(scope="module")
def grid_cases(orbx_lib):
    return fc.grid_cases()


# ---- restatement agreement ---------------------------------------------------------------------------

def test_grid_restatements_agree(oracle_mod, grid_cases):
    from oracle import matcher as om
    batch = fc.grid_batch_case()
    s = batch["stride"]
    frames = [dict(batch, name=f"batch{f}", keys=batch["keys"][f * s:f * s + int(n)])
              for f, n in enumerate(batch["counts"])]
    for c, ref in zip(grid_cases + frames, [fc.grid_reference(c) for c in grid_cases] +
                      [r + (None,) for r in fc.grid_batch_reference(batch)]):
        off, feat, _ = ref
        o_off, o_feat = om.assign_grid(c["keys"], c["min_x"], c["min_y"], c["inv_w"], c["inv_h"],
                                       c["cols"], c["rows"])
        np.testing.assert_array_equal(off, o_off, c["name"])
        np.testing.assert_array_equal(feat, o_feat, c["name"])
        if (c["cols"], c["rows"]) == (64, 48):
            with np.errstate(invalid="ignore"):
                g = assign_features_to_grid(c["keys"], *c["bounds"])
            assert (f32(g.inv_w), f32(g.inv_h)) == (c["inv_w"], c["inv_h"])
            np.testing.assert_array_equal(off, g.off, c["name"])
            np.testing.assert_array_equal(feat, g.feat, c["name"])


def test_undistort_restatements_agree(oracle_mod):
    from oracle import matcher as om
    for c in fc.undistort_cases() + [fc.undistort_batch_case(cam) for cam in fc.UNDIST_CAMS]:
        if len(c["keys"]) == 0:
            continue
        want = fc.undistort_ref(c["keys"], c["K4"], c["dist"])
        got = om.undistort_keypoints(c["keys"], c["K4"], c["dist"])
        # NaN canonised: float fields only (x, y)
        assert fc.canon_keys(want)[:, :2].tobytes() == fc.canon_keys(
            fc.kp(got[:, 0], got[:, 1]))[:, :2].tobytes(), c["name"]
        for f in ("size", "angle", "response", "octave", "class_id"):
            assert want[f].tobytes() == c["keys"][f].tobytes()


def test_gray_restatements_agree(oracle_mod):
    from oracle import matcher as om
    for c in fc.gray_cases():
        np.testing.assert_array_equal(fc.gray_np(c["img"], c["rgb"]), om.cvt_gray(c["img"], c["rgb"]), c["name"])
        if c["img"].shape[2] == 4:
            np.testing.assert_array_equal(fc.gray_np(fc.with_other_alpha(c["img"]), c["rgb"]),
                                          fc.gray_np(c["img"], c["rgb"]))
    img = fc.exhaustive_image()
    assert len(np.unique(img.reshape(-1, 3).astype(np.uint32) @ np.array([1, 256, 65536], np.uint32))) == 1 << 24
    for rgb in (0, 1):
        want = fc.gray_np(img, rgb)
        np.testing.assert_array_equal(want, om.cvt_gray(img, rgb))
        assert want.min() == 0 and want.max() == 255


def test_frustum_restatements_agree(oracle_mod):
    from oracle import matcher as om
    cases = fc.frustum_cases()
    b = fc.frustum_batch_case()
    cases = cases + [fc._fcase(f"batch{k}", F, m, s) for k, (F, m, s) in enumerate(zip(b["frames"], b["mps"], b["skip"]))]
    for c in cases:
        q, n, _ = fc.frustum_np(c["F"], c["mps"], c["skip"], c["cos_lim"], c["th"])
        qo, no = om.is_in_frustum(c["F"], c["mps"], c["skip"], c["cos_lim"], c["th"])
        assert n == no == int((q["radius"] >= 0).sum()), c["name"]
        # x86's 0 * inf is the negative quiet NaN; the float fields are canonised on both sides
        bad = np.nonzero((fc.canon_queries(q) != fc.canon_queries(qo)).any(1))[0]
        assert bad.size == 0, f"{c['name']}: queries differ at points {bad[:8]}"


# ---- census: what the cases contain, on the restatement alone ------------------------------------------

def _gcase(cases, name):
    (c,) = [c for c in cases if c["name"] == name]
    return c, fc.grid_reference(c)


def test_grid_census(grid_cases):
    c, (off, feat, info) = _gcase(grid_cases, "exact_halves")
    half = (info["vx"] - np.floor(info["vx"])) == 0.5
    pos_half = half & (info["vx"] > 0) & (info["cell"] >= 0)
    # with bounds (0, 512, 0, 384): x = 4 -> column 1, x = -4 outside, x = 500 -> 63, x = 508 outside
    x = c["keys"]["x"]
    for xv, col in ((4.0, 1), (-4.0, None), (500.0, 63), (508.0, None)):
        (i,) = np.nonzero((x == f32(xv)) & (c["keys"]["y"] == 101.0))
        assert (info["cell"][i[0]] // 48 == col) if col is not None else info["cell"][i[0]] == -1, xv
    assert set(info["px"][pos_half].tolist()) == set(range(1, 64))          # every column by a half
    halfy = ((info["vy"] - np.floor(info["vy"])) == 0.5) & (info["vy"] > 0) & (info["cell"] >= 0)
    assert set(info["py"][halfy].tolist()) == set(range(1, 48))
    assert ((info["vx"] == -0.5) & (info["cell"] == -1)).any() and ((info["vy"] == -0.5) & (info["cell"] == -1)).any()
    # the realistic bounds hold exact halves too, and both sides of every boundary
    n_half = {}
    for cam in fc.CAMS:
        c, (off, feat, info) = _gcase(grid_cases, f"boundaries_{cam}")
        hx = ((info["vx"] - np.floor(info["vx"])) == 0.5) & (info["vx"] > 0) & (info["cell"] >= 0)
        n_half[cam] = int(hx[:130].sum())
        px, py = info["px"][:130].reshape(-1, 2), info["py"][130:].reshape(-1, 2)
        assert (px[:, 0] == np.arange(-1, 64)).all() and (px[:, 1] == np.arange(0, 65)).all()
        assert (py[:, 0] == np.arange(-1, 48)).all() and (py[:, 1] == np.arange(0, 49)).all()
        x = c["keys"]["x"][:130].reshape(-1, 2)
        assert (np.nextafter(x[:, 0], f32(np.inf)) == x[:, 1]).all()
    assert n_half["euroc"] >= 10, n_half
    # first / last column and row
    cells = np.concatenate([fc.grid_reference(c)[2]["cell"] for c in grid_cases if (c["cols"], c["rows"]) == (64, 48)])
    cells = cells[cells >= 0]
    assert {0, 63} <= set((cells // 48).tolist()) and {0, 47} <= set((cells % 48).tolist())
    for cols, rows in fc.GRID_SHAPES:
        _, (off, feat, info) = _gcase(grid_cases, f"shape_{cols}x{rows}")
        cl = info["cell"][info["cell"] >= 0]
        assert {0, cols - 1} <= set((cl // rows).tolist()) and {0, rows - 1} <= set((cl % rows).tolist())
        assert 0 < len(feat) < len(info["cell"])
    # a crowded cell, an empty grid, one feature per cell
    _, (off, feat, _) = _gcase(grid_cases, "one_cell_2048")
    assert np.diff(off).max() == 2048 and (feat == np.arange(2048)).all()
    _, (off, feat, _) = _gcase(grid_cases, "all_outside")
    assert len(feat) == 0 and (off == 0).all()
    _, (off, feat, _) = _gcase(grid_cases, "every_cell_once")
    assert (np.diff(off) == 1).all() and (feat != np.arange(3072)).any()
    for n in fc.GRID_COUNTS:
        assert len(_gcase(grid_cases, f"count_{n}")[0]["keys"]) == n
    # each non-finite kind, in x and in y, is excluded; -0.0 is column 0 of the exact grid
    for name in ("nonfinite_exact", "nonfinite_euroc"):
        c, (off, feat, info) = _gcase(grid_cases, name)
        k = c["keys"]
        for axis in ("x", "y"):
            for pred in (np.isnan, np.isposinf, np.isneginf, lambda a: a == f32(3e9),
                         lambda a: a == f32(-3e9), lambda a: a == f32(1e30), lambda a: a == f32(-1e30)):
                hit = pred(k[axis])
                assert hit.any() and (info["cell"][hit] == -1).all(), (name, axis)
        assert (np.isnan(k["x"]) & np.isnan(k["y"])).any()
        assert (np.isnan(k["x"]) & ~np.isnan(k["y"])).any() and (~np.isnan(k["x"]) & np.isnan(k["y"])).any()
        assert info["cell"][-1] >= 0                       # the finite control point is inside
    c, (off, feat, info) = _gcase(grid_cases, "nonfinite_exact")
    i = int(np.nonzero((c["keys"]["x"] == 0) & np.signbit(c["keys"]["x"]))[0][0])
    assert info["px"][i] == 0 and info["cell"][i] >= 0
    # the batch: pad slots inside the grid, counts on both clamps
    b = fc.grid_batch_case()
    assert b["counts"].tolist() == [1024, 0, 1100, 0, 1, 1100]
    assert [len(f) for _, f in fc.grid_batch_reference(b)] == b["counts"].tolist()
    assert len(fc.grid_np(b["keys"], 64, 48, b["min_x"], b["min_y"], b["inv_w"], b["inv_h"])[1]) == len(b["keys"])


def test_undistort_census():
    cases = {c["name"]: c for c in fc.undistort_cases()}
    assert {len(c["keys"]) for c in cases.values()} == set(fc.UNDIST_COUNTS)
    for cam, (K4, dist) in fc.UNDIST_CAMS.items():
        k = cases[f"{cam}_n257"]["keys"]
        assert [(float(a), float(b)) for a, b in zip(k["x"][:4], k["y"][:4])] == list(fc.CORNERS)
        assert k["x"][4] == f32(K4[2]) and k["y"][4] == f32(K4[3])
        assert (k["x"] > 1e4).any() and (k["x"] < -9e3).any() and (k["y"] > 1e4).any() and (k["y"] < -9e3).any()
        un = fc.undistort_ref(k, K4, dist)
        if cam == "copy":
            assert dist[0] == 0 and any(d != 0 for d in dist[1:]) and un.tobytes() == k.tobytes()
        else:
            assert (un["x"][:5] != k["x"][:5]).sum() >= 4
    _, _, den = fc.pole_point(*fc.UNDIST_CAMS["rational_pole"])
    assert abs(den) < 1e-6
    k = cases["rational_pole_n257"]["keys"]
    un = fc.undistort_ref(k, *fc.UNDIST_CAMS["rational_pole"])
    assert not np.isfinite(un["x"]).all()                  # non-finite results are legitimate
    b = fc.undistort_batch_case("euroc")
    assert b["counts"].tolist() == [257, 0, 300, 0, 1, 300]


def test_frustum_census():
    cases = fc.frustum_cases()
    refs = {c["name"]: (c, fc.frustum_reference(c)) for c in cases}
    seen = set()
    for c, (q, n, info) in refs.values():
        seen |= set(info["outcome"])
    assert seen == set(fc.FRUSTUM_OUTCOMES)
    up, dn = fc.up, fc.dn
    # depth: the four values around zero, and a NaN u that is accepted
    c, (q, n, info) = refs["depth"]
    z, out = info["z"], info["outcome"]
    assert ((z == 0) & np.signbit(z)).any() and ((z == 0) & ~np.signbit(z)).any()
    assert (z == f32(1.4e-45)).any() and (z == f32(-1.4e-45)).any()
    assert all(o == "depth" for o, zz in zip(out, z) if zz < 0) and "depth" in out
    assert out[0] == "u_high" and np.signbit(z[0])           # -0.0 passes the depth test
    assert out[1] == "visible" and z[1] == 0 and np.isnan(q["u"][1]) and np.isnan(q["v"][1])
    assert info["dist"][1] == 0                              # the point at Ow
    # u / v on each bound and one float either side, in both frames
    for name in ("bounds", "bounds_shifted"):
        c, (q, n, info) = refs[name]
        F = c["F"]
        for key, lo, hi, rej in (("u", F["min_x"], F["max_x"], ("u_low", "u_high")),
                                 ("v", F["min_y"], F["max_y"], ("v_low", "v_high"))):
            val, out = info[key], np.array(info["outcome"])
            for t, o in ((dn(lo), rej[0]), (lo, "visible"), (up(lo), "visible"), (dn(hi), "visible"),
                         (hi, "visible"), (up(hi), rej[1])):
                hit = val == t
                assert hit.any() and (out[hit] == o).any(), (name, key, float(t), o)
    # dist on both thresholds and one float either side; dist = 0; max_dist 0 and inf
    for name in ("dist", "dist_shifted"):
        c, (q, n, info) = refs[name]
        d, out, m = info["dist"], np.array(info["outcome"]), c["mps"]
        lo, hi = f32(0.8) * m["min_dist"], f32(1.2) * m["max_dist"]
        assert ((d == lo) & (lo > 0) & (out == "visible")).any() and ((d == hi) & (out == "visible")).any()
        assert ((d == dn(lo)) & (out == "dist_low")).any() and ((d == up(lo)) & (lo > 0) & (out == "visible")).any()
        assert ((d == up(hi)) & (out == "dist_high")).any() and ((d == dn(hi)) & (hi > 0) & (out == "visible")).any()
    c, (q, n, info) = refs["dist"]
    m, out = c["mps"], np.array(info["outcome"])
    assert ((m["max_dist"] == 0) & (info["dist"] == 0) & (out == "visible")).any()
    assert ((m["max_dist"] == 0) & (info["dist"] > 0) & (out == "dist_high")).any()
    assert (np.isposinf(m["max_dist"]) & (out == "visible")).any()
    # viewCos on the limit and around it, around 0.998: both radii
    for cl in (0.5, 0.25, 0.7):
        c, (q, n, info) = refs[f"viewcos_{cl}"]
        vc, out = info["vc"], np.array(info["outcome"])
        assert out[vc == f32(cl)].tolist() == ["visible"] and out[vc == dn(cl)].tolist() == ["viewcos"]
        assert out[vc == up(cl)].tolist() == ["visible"]
        assert info["r0"][vc == fc.LO998] == 4.0 and info["r0"][vc == fc.HI998] == 2.5
        assert float(fc.LO998) < 0.998 < float(fc.HI998) and up(fc.LO998) == fc.HI998
    # PredictScale: every level, both clamps, quotients on integers and either side
    for nl in (1, 8, 16):
        c, (q, n, info) = refs[f"level_nl{nl}"]
        quot, lv = info["quot"], q["pred_level"]
        assert set(lv.tolist()) == set(range(nl)) and "above" in info["clamp"]
        exact = [L for L in range(nl + 1) if (quot == L).any()]
        assert {0, 1} <= set(exact), exact
        for L in range(nl + 1):                             # the two sides of every ceil step
            assert ((quot <= L) & (quot > L - 0.001)).any() and ((quot > L) & (quot < L + 0.001)).any()
        c, (q, n, info) = refs[f"level_clamp_nl{nl}"]
        assert "below" in info["clamp"] and "above" in info["clamp"] and (info["quot"] < -1).any()
        assert q["pred_level"].max() == nl - 1 and q["pred_level"].min() == 0
    # th applied and not applied
    assert not refs["th_1.0"][1][2]["th_applied"].any()
    for name in ("th_3.0", f"th_{fc.TH1UP!r}"):
        c, (q, n, info) = refs[name]
        assert info["th_applied"].all() and set(info["r0"].tolist()) == {2.5, 4.0}
    # skip flags and counts
    assert refs["skip_none"][0]["skip"] is None and refs["skip_none"][1][1] == 41
    assert refs["skip_zeros"][1][1] == 41 and refs["skip_ones"][1][1] == 0 and refs["skip_alt"][1][1] == 21
    for n in fc.FRUSTUM_COUNTS:
        assert refs[f"count_all_{n}"][1][1] == n and refs[f"count_last_{n}"][1][1] == 1
        assert refs[f"count_last_{n}"][1][0]["radius"][-1] > 0
    b = fc.frustum_batch_case()
    assert [len(m) for m in b["mps"]] == [257, 0, 1, 0, 64]


# ---- variants: every plausible mistake moves a directed case ------------------------------------------

@pytest.mark.parametrize("variant", fc.GRID_VARIANTS)
def test_grid_variant_changes_a_case(grid_cases, variant):
    changed = []
    for c in grid_cases:
        if c["name"].startswith(("count_", "every_cell")) and variant != "no_sort":
            continue
        off, feat, _ = fc.grid_reference(c)
        voff, vfeat, _ = fc.grid_np(c["keys"], c["cols"], c["rows"], c["min_x"], c["min_y"], c["inv_w"],
                                    c["inv_h"], variant)
        if off.tobytes() != voff.tobytes() or feat.tobytes() != vfeat.tobytes():
            changed.append(c["name"])
    assert changed, variant
    pins = {"rint": "exact_halves", "trunc": "exact_halves", "nan_zero": "nonfinite_exact",
            "px_le_cols": "edges_exact", "no_sort": "one_cell_2048"}
    if variant in pins:
        assert pins[variant] in changed, (variant, changed)


@pytest.mark.parametrize("variant", fc.UNDIST_VARIANTS)
def test_undistort_variant_changes_a_case(variant):
    changed = [c["name"] for c in fc.undistort_cases() if
               fc.canon_keys(fc.undistort_ref(c["keys"], c["K4"], c["dist"])).tobytes() !=
               fc.canon_keys(fc.undistort_ref(c["keys"], c["K4"], c["dist"], variant)).tobytes()]
    assert changed, variant
    if variant == "copy_all_zero":
        assert all(n.startswith("copy_") for n in changed)


@pytest.mark.parametrize("variant", fc.GRAY_VARIANTS)
def test_gray_variant_changes_a_case(variant):
    changed = [c["name"] for c in fc.gray_cases()
               if (fc.gray_np(c["img"], c["rgb"]) != fc.gray_np(c["img"], c["rgb"], variant)).any()]
    assert changed, variant
    assert any("_c4_" in n for n in changed)


@pytest.mark.parametrize("variant", fc.FRUSTUM_VARIANTS)
def test_frustum_variant_changes_a_case(variant):
    changed = []
    for c in fc.frustum_cases():
        q, n, _ = fc.frustum_reference(c)
        qv, nv, _ = fc.frustum_np(c["F"], c["mps"], c["skip"], c["cos_lim"], c["th"], variant)
        if (fc.canon_queries(q) != fc.canon_queries(qv)).any() or n != nv:
            changed.append(c["name"])
    assert changed, variant
    pins = {"u_low_le": "bounds", "u_high_ge": "bounds", "v_low_le": "bounds", "v_high_ge": "bounds",
            "dist_low_le": "dist", "dist_high_ge": "dist", "viewcos_le": "viewcos_0.5", "z_le": "depth",
            "f998": "viewcos_0.5", "floor": "level_nl8", "th_never": "th_3.0",
            "th_eps": f"th_{fc.TH1UP!r}", "no_clamp_above": "level_nl8", "ur_plus": "th_1.0"}
    assert pins[variant] in changed, (variant, changed)
    if variant in ("u_low_le", "u_high_ge", "v_low_le", "v_high_ge"):
        assert "bounds_shifted" in changed
    if variant in ("dist_low_le", "dist_high_ge"):
        assert "dist_shifted" in changed


def test_th_multiplied_unconditionally_is_the_same_function():
    """Why no variant 'th multiplied unconditionally': r * 1.0f is r for both radii, so it cannot
    change a query; the condition is pinned by th_never and th_eps instead."""
    for r in (f32(2.5), f32(4.0)):
        assert f32(r * f32(1.0)).tobytes() == r.tobytes()


# ---- the C ABI without a GPU ------------------------------------------------------------------------------

def test_grid_refusals_need_no_gpu(orbx_lib):
    """More than 15360 cells (64 KiB of LDS with the scan partials) is ORBX_ERR_INVALID, decided
    before the device is touched; nothing is written."""
    L = orbx_lib
    keys = fc.kp([1.0, 2.0], [1.0, 2.0])
    off = np.full(121 * 127 + 1, -7, np.int32)
    feat = np.full(2, -7, np.int32)
    dn_ = np.array([2], np.int32)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)
    for cols, rows in ((121, 127), (15361, 1), (0, 48), (64, -1), (65536, 65536)):
        assert L.orbx_assign_grid_device(P(keys), 2, cols, rows, 0.0, 0.0, 0.125, 0.125, P(off), P(feat), None) == -1
        assert L.orbx_assign_grid_batch_device(P(keys), 2, P(dn_), 1, cols, rows, 0.0, 0.0, 0.125, 0.125,
                                               P(off), P(feat), None) == -1
    assert L.orbx_assign_grid_device(P(keys), -1, 64, 48, 0.0, 0.0, 0.125, 0.125, P(off), P(feat), None) == -1
    assert L.orbx_assign_grid_device(P(keys), 2, 64, 48, 0.0, 0.0, 0.125, 0.125, None, P(feat), None) == -1
    assert (off == -7).all() and (feat == -7).all()
