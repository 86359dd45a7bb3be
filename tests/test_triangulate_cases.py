"""CPU: the loop body of LocalMapping::CreateNewMapPoints that orbx_triangulate_matches* runs
(tests/triangulate_cases.py).  The numpy restatement against the cv::Mat restatement of
tests/native/triangulate_ref.cpp, bit for bit, on every directed and random case; the census of
what the cases contain; every single-decision variant changes a case; the restated hypot against
the C library's; orbx_parallax_stereo_cos against numpy; the C ABI's argument checks, which need
no GPU; and, independent of the restatements being right, the restated SVD and x3D against
numpy.linalg.svd in float64."""
import ctypes
import subprocess

import numpy as np
import pytest

import triangulate_cases as tc
from my_orb_slam2_amd.features import FRAME_POSE_DTYPE

f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def triangulate_ref():
    from my_orb_slam2_amd import build as b
    return b.build_triangulate_ref()


def run_ref(binary, cases, tmp_path):
    """The C++ restatement on a list of cases -> [(status, x3d)]."""
    src, dst = tmp_path / "cases.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for c in cases:
            n1, n2, m = len(c["keys1"]), len(c["keys2"]), len(c["pairs"])
            flags = sum(bit for bit, k in ((1, "raw1"), (2, "raw2"), (4, "ur1"), (8, "ur2"))
                        if c.get(k) is not None)
            f.write(np.array([n1, n2, m, flags], np.int32).tobytes())
            f.write(f32(c["ratio_factor"]).tobytes())
            f.write(np.asarray(c["pose1"], FRAME_POSE_DTYPE).tobytes())
            f.write(np.asarray(c["pose2"], FRAME_POSE_DTYPE).tobytes())
            f.write(c["keys1"].tobytes() + c["keys2"].tobytes())
            for k in ("raw1", "raw2", "ur1", "ur2"):
                if c.get(k) is not None:
                    f.write(np.ascontiguousarray(c[k]).tobytes())
            for k, n in (("depth1", n1), ("depth2", n2)):
                f.write((np.zeros(n, f32) if c.get(k) is None else np.asarray(c[k], f32)).tobytes())
            c1, c2 = tc.cos_tables(c)
            f.write(c1.tobytes() + c2.tobytes())
            f.write(np.asarray(c["pairs"], np.int32).tobytes())
    subprocess.run([str(binary), str(src), str(dst)], check=True, timeout=120)
    raw = dst.read_bytes()
    out, o = [], 0
    for c in cases:
        m = len(c["pairs"])
        st = np.frombuffer(raw, np.int32, m, o)
        o += 4 * m
        out.append((st, np.frombuffer(raw, f32, 3 * m, o).reshape(m, 3)))
        o += 12 * m
    assert o == len(raw)
    return out


def test_numpy_equals_cv_mat_restatement(triangulate_ref, tmp_path):
    cases = tc.all_cases()
    for c, (st_ref, x_ref) in zip(cases, run_ref(triangulate_ref, cases, tmp_path)):
        st, x, _ = tc.reference(c)
        assert np.array_equal(st, st_ref), (c["name"], st.tolist(), st_ref.tolist())
        ok = st <= tc.OK_STEREO2
        assert x[ok].tobytes() == x_ref[ok].tobytes(), c["name"]
        assert not np.isnan(x[ok]).any(), c["name"]


def test_restated_hypot_equals_the_c_library(triangulate_ref):
    """glibc 2.35's hypot as the kernel and the C++ restatement write it (the form without a
    fused multiply-add), against the host's C library over the whole exponent range."""
    r = subprocess.run([str(triangulate_ref), "--hypot", "1000000", "3"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


def test_level_sigma2_is_the_squared_scale_factor(oracle_mod):
    """mvLevelSigma2[o] = mvScaleFactor[o] * mvScaleFactor[o] in float (ORBextractor.cc:421-422):
    what the kernel computes from orbx_frame_pose.scale, against the extractor's own tables."""
    for factor, nlevels in ((1.2, 8), (1.2, 16), (1.5, 5), (1.1, 12)):
        t = oracle_mod.OracleExtractor(500, factor, nlevels, 20, 7).tables()
        assert (t["scale"] * t["scale"]).tobytes() == t["sigma2"].tobytes()
        assert t["scale"].tobytes() == tc.scale_factors(nlevels, factor).tobytes()


# ---- the census -----------------------------------------------------------------------------------

def _codes(name):
    return [tc.CODES[k] for k in tc.reference(tc.case_named(name))[0]]


def test_census_every_outcome_occurs():
    seen, directed, combos = set(), set(), set()
    for c in tc.all_cases():
        st, _, infos = tc.reference(c)
        seen |= set(st.tolist())
        if not c["name"].startswith("random"):
            directed |= set(st.tolist())
        ur1 = np.full(len(c["keys1"]), -1, f32) if c["ur1"] is None else c["ur1"]
        ur2 = np.full(len(c["keys2"]), -1, f32) if c["ur2"] is None else c["ur2"]
        for (i1, i2), code in zip(c["pairs"], st):
            combos.add((bool(ur1[i1] >= 0), bool(ur2[i2] >= 0), int(code) <= tc.OK_STEREO2))
    assert seen == set(tc.LOOP_CODES), set(tc.LOOP_CODES) - seen
    assert directed == set(tc.LOOP_CODES), "the directed cases alone reach every exit"
    # each (bStereo1, bStereo2) combination both succeeds and fails somewhere
    assert combos == {(a, b, ok) for a in (False, True) for b in (False, True) for ok in (False, True)}


def test_census_named_constructs():
    # the four stereo combinations: with parallax the SVD branch, without it each own branch
    for tag in ("st00", "st01", "st10", "st11"):
        assert set(_codes("near_" + tag)) == {"OK_TRIANGULATED"}
    assert set(_codes("small_baseline_st00")) == {"LOW_PARALLAX"}
    assert set(_codes("small_baseline_st10")) == {"OK_STEREO1"}
    assert set(_codes("small_baseline_st01")) == {"OK_STEREO2"}
    assert set(_codes("small_baseline_st11")) == {"OK_STEREO1"}
    # the quirks: the outcome differs without them
    c = tc.case_named("quirk_388")
    assert _codes("quirk_388") == ["OK_TRIANGULATED"]
    assert tc.triangulate_np(c, "if_388")[0].tolist() == [tc.OK_STEREO2]
    c = tc.case_named("quirk_482")
    assert set(_codes("quirk_482")) == {"OK_TRIANGULATED"}
    assert set(tc.triangulate_np(c, "mbf2_482")[0].tolist()) == {tc.REPROJ_2}
    assert set(_codes("quirk_482_own_mbf")) == {"REPROJ_2"}
    # rank-deficient A, the point at a camera centre
    for name in ("equal_poses_rank3", "equal_poses_rank2_stereo"):
        c = tc.case_named(name)
        assert c["pose1"].tobytes() == c["pose2"].tobytes()
        for info in tc.reference(c)[2]:
            s = np.linalg.svd(info["A"].astype(f64), compute_uv=False)
            assert s[3] < 1e-6 * s[0] and (name.endswith("rank3") or s[2] < 1e-6 * s[0])
    st, _, infos = tc.reference(tc.case_named("equal_poses_rank3"))
    for info in infos:                       # the null vector is the camera centre (0, 0, 0, 1)
        v = info["v"] / info["v"][3]
        assert np.abs(v[:3]).max() < 1e-5
    assert _codes("w_zero") == ["W_ZERO"]
    assert tc.reference(tc.case_named("w_zero"))[2][0]["v"][3] == 0
    # octaves 0 and nlevels - 1
    for name in ("octaves_0_7", "octaves_7_0", "octaves_7_7"):
        c = tc.case_named(name)
        assert {0, tc.NLEVELS - 1} >= set(c["keys1"]["octave"]) | set(c["keys2"]["octave"])
    assert set(_codes("octaves_0_7")) == set(_codes("octaves_7_0")) == {"SCALE"}
    assert tc.triangulate_np(tc.case_named("octaves_0_7"), "remove:scale_high")[0].tolist() == [0] * 4
    assert tc.triangulate_np(tc.case_named("octaves_7_0"), "remove:scale_low")[0].tolist() == [0] * 4
    # z == 0 and dist == 0 exactly
    assert tc.triangulate_np(tc.case_named("z1_zero"), "behind_1_strict")[0][0] != tc.BEHIND_1
    assert tc.triangulate_np(tc.case_named("z2_zero"), "behind_2_strict")[0][0] != tc.BEHIND_2
    assert _codes("dist1_zero") == _codes("dist2_zero") == ["DIST_ZERO"]
    assert "REPROJ_2" in _codes("reproj_2_mono") and "REPROJ_1" in _codes("reproj_1_6px_o0")
    assert set(_codes("reproj_stereo_1_4px")) == {"REPROJ_1"}
    assert set(_codes("reproj_stereo_2_4px")) == {"REPROJ_2"}
    assert set(_codes("stereo_without_depth")) == {"LOW_PARALLAX"}
    c = tc.case_named("raw_keys")
    assert set(_codes("raw_keys")) == {"OK_STEREO1"}
    assert tc.reference(c)[1].tobytes() != tc.triangulate_np(dict(c, raw1=None))[1].tobytes()


def test_census_thresholds_of_cos_parallax_rays():
    up = lambda a: np.nextafter(f32(a), f32(np.inf))
    dn = lambda a: np.nextafter(f32(a), f32(-np.inf))
    # cosParallaxStereo: `<` is strict, on either side's table
    for k in ("1", "2"):
        cr = [tc.reference(tc.case_named(f"threshold_stereo{k}_{t}"))[2][0]["cos_rays"]
              for t in ("below", "equal", "above")]
        assert cr[0] == cr[1] == cr[2]
        tab = [tc.case_named(f"threshold_stereo{k}_{t}")["cos" + k][0] for t in ("below", "equal", "above")]
        assert tab == [dn(cr[0]), cr[0], up(cr[0])]
        ok = "OK_STEREO" + k
        assert [_codes(f"threshold_stereo{k}_{t}")[0] for t in ("below", "equal", "above")] == \
            [ok, ok, "OK_TRIANGULATED"]
    # 0.9998 is a double between two floats: the float above it fails, the one below passes
    hi = tc.reference(tc.case_named("threshold_9998_at_or_above"))[2][0]["cos_rays"]
    lo = tc.reference(tc.case_named("threshold_9998_below"))[2][0]["cos_rays"]
    assert hi == f32(0.9998) and lo == dn(hi) and float(lo) < 0.9998 < float(hi)
    assert _codes("threshold_9998_at_or_above") == ["LOW_PARALLAX"]
    assert _codes("threshold_9998_below") == ["OK_TRIANGULATED"]
    # 0: the least denormal either side
    cr = [tc.reference(tc.case_named(f"threshold_0_{t}"))[2][0]["cos_rays"] for t in ("neg", "zero", "pos")]
    assert cr[0] == dn(0) and cr[1] == 0 and cr[2] == up(0)
    assert [_codes(f"threshold_0_{t}")[0] for t in ("neg", "zero", "pos")][:2] == ["LOW_PARALLAX"] * 2
    assert _codes("threshold_0_pos")[0] != "LOW_PARALLAX"
    assert tc.triangulate_np(tc.case_named("threshold_0_zero"), "cos_gt_0_nonstrict")[0][0] != tc.LOW_PARALLAX


def _variant_cases():
    # two random scenes are enough here
    return [c for c in tc.all_cases() if not c["name"].startswith("random")
            or c["name"] in ("random11", "random15")]


@pytest.mark.parametrize("variant", tc.VARIANTS)
def test_every_variant_changes_a_case(variant):
    """Each decision of the restatement is pinned: switching it changes at least one case."""
    changed = []
    for c in _variant_cases():
        st, x, _ = tc.reference(c)
        sv, xv, _ = tc.triangulate_np(c, variant)
        if st.tobytes() != sv.tobytes() or x.tobytes() != xv.tobytes():
            changed.append(c["name"])
    assert changed, f"{variant} changes nothing"


def test_directed_variant_pins():
    """The directed cases, not only the random ones, pin the decisions they were built for."""
    def differs(name, variant):
        c = tc.case_named(name)
        return tc.reference(c)[0].tobytes() != tc.triangulate_np(c, variant)[0].tobytes()
    assert differs("quirk_388", "if_388") and differs("quirk_482", "mbf2_482")
    assert differs("threshold_stereo1_equal", "cos_lt_stereo_nonstrict")
    assert differs("threshold_stereo2_equal", "cos_lt_stereo_nonstrict")
    assert differs("threshold_0_zero", "cos_gt_0_nonstrict")
    assert differs("threshold_9998_at_or_above", "remove:parallax_gate")
    assert differs("z1_zero", "behind_1_strict") and differs("z2_zero", "behind_2_strict")
    assert differs("w_zero", "remove:w_zero")
    assert differs("dist1_zero", "remove:dist_zero") and differs("dist2_zero", "remove:dist_zero")
    assert differs("behind_1", "remove:behind_1") and differs("behind_2", "remove:behind_2")
    assert differs("reproj_1_6px_o0", "remove:reproj_1") and differs("reproj_2_mono", "remove:reproj_2")
    assert differs("small_baseline_st10", "remove:stereo1_select")
    assert differs("small_baseline_st01", "remove:stereo2_select")


# ---- orbx_parallax_stereo_cos ---------------------------------------------------------------------

def test_parallax_stereo_cos_equals_numpy(orbx_lib):
    from my_orb_slam2_amd.matcher import parallax_stereo_cos
    depths = [c[k] for c in tc.all_cases() for k in ("depth1", "depth2") if c.get(k) is not None]
    rng = np.random.default_rng(5)
    depths.append(np.array([0.0, -0.0, -1.0, np.inf, -np.inf, 1e-30, 1e30, np.nan], f32))
    depths.append(rng.uniform(0.05, 80, 20000).astype(f32))
    d = np.concatenate(depths).astype(f32)
    for mb in (tc.MB, f32(0.11), f32(0.5372), f32(0)):
        got = parallax_stereo_cos(mb, d)
        want = tc.stereo_cos_np(mb, d)
        assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    assert parallax_stereo_cos(0.1, np.zeros(0, f32)).shape == (0,)


# ---- the C ABI without a GPU ----------------------------------------------------------------------

def _abi(orbx_lib, case, **over):
    """orbx_triangulate_matches on a case with single arguments replaced -> status code."""
    P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    keep = dict(pose1=np.asarray(case["pose1"], FRAME_POSE_DTYPE).copy(),
                pose2=np.asarray(case["pose2"], FRAME_POSE_DTYPE).copy(),
                keys1=case["keys1"].copy(), keys2=case["keys2"].copy(), ur1=case["ur1"],
                ur2=case["ur2"], depth1=case["depth1"], depth2=case["depth2"],
                pairs=np.ascontiguousarray(case["pairs"], np.int32), mb=float(case["mb"]),
                n1=len(case["keys1"]), n2=len(case["keys2"]), npairs=len(case["pairs"]))
    keep.update(over)
    k = keep
    m = max(k["npairs"], 1)
    status, x3d, nnew = np.zeros(m, np.int32), np.zeros(3 * m, f32), ctypes.c_int32(-7)
    k.setdefault("status", status)
    k.setdefault("x3d", x3d)
    rc = orbx_lib.orbx_triangulate_matches(
        P(k["pose1"]), P(k["pose2"]), P(k["keys1"]), None, P(k["ur1"]), P(k["depth1"]), None,
        k["n1"], P(k["keys2"]), None, P(k["ur2"]), P(k["depth2"]), None, k["n2"], k["mb"],
        float(case["ratio_factor"]), P(k["pairs"]), k["npairs"], P(k["status"]), P(k["x3d"]),
        ctypes.byref(nnew), 0)
    return rc, nnew.value


def test_symbols_and_argument_statuses_need_no_gpu(orbx_lib):
    """Every argument check is decided before the device is touched."""
    import torch
    L = orbx_lib
    for name in ("orbx_triangulate_matches", "orbx_triangulate_matches_batch_device",
                 "orbx_parallax_stereo_cos"):
        assert hasattr(L, name)
    INVALID, UNSUPPORTED = -1, -4
    c = tc.case_named("near_st11")
    bad = lambda **kw: _abi(L, c, **kw)[0]
    for null in ("pose1", "pose2", "keys1", "keys2", "pairs", "status", "x3d"):
        assert bad(**{null: None}) == INVALID, null
    assert bad(depth1=None) == INVALID and bad(depth2=None) == INVALID     # u_right without depth
    assert bad(n1=-1) == INVALID and bad(n2=-1) == INVALID and bad(npairs=-1) == INVALID
    assert bad(mb=-0.5) == INVALID and bad(mb=float("nan")) == INVALID
    pr = np.ascontiguousarray(c["pairs"], np.int32)
    for p, v in ((0, -1), (0, len(c["keys1"])), (1, -1), (1, len(c["keys2"]))):
        q = pr.copy()
        q[1, p] = v
        assert bad(pairs=q) == INVALID                                     # outside its keyframe
    q = pr.copy()
    q[2, 0] = q[1, 0]
    assert bad(pairs=q) == INVALID                                         # idx1 twice
    for which in ("keys1", "keys2"):
        for octave in (-1, tc.NLEVELS, 1 << 20):
            k = c[which].copy()
            k["octave"][int(pr[0, 0])] = octave
            assert bad(**{which: k}) == INVALID                            # octave >= nlevels
    for which in ("pose1", "pose2"):
        for nl, want in ((0, INVALID), (-2, INVALID), (17, UNSUPPORTED)):
            F = np.asarray(c[which], FRAME_POSE_DTYPE).copy()
            F["nlevels"] = nl
            assert bad(**{which: F}) == want
    assert bad(n1=32769) == UNSUPPORTED
    # nothing to do: no device needed either
    assert _abi(L, c, npairs=0) == (0, 0)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)
    d = np.zeros(4, f32)
    assert L.orbx_parallax_stereo_cos(0.1, None, 4, P(d)) == INVALID
    assert L.orbx_parallax_stereo_cos(0.1, P(d), -1, P(d)) == INVALID
    assert L.orbx_triangulate_matches_batch_device(None, None, 1, *([None] * 6), 0.1, 1.8,
                                                   *([None] * 6)) == INVALID     # no matcher
    if not torch.cuda.is_available():
        assert _abi(L, c)[0] == -2                                          # ORBX_ERR_DEVICE


def test_without_gpu_the_host_form_fails_loudly(orbx_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    import my_orb_slam2_amd as m
    c = tc.case_named("near_st00")
    with pytest.raises(m.OrbxError) as e:
        m.triangulate_matches(c["pose1"], c["pose2"], c["keys1"], c["keys2"], c["pairs"],
                              c["ratio_factor"])
    assert e.value.code == -2     # ORBX_ERR_DEVICE


# ---- independent of the restatements: float64 ------------------------------------------------------

# A case is left out of the vector comparisons when its two smallest float64 singular values are
# within a factor GAP_RATIO of each other: the smallest right singular vector is then not
# determined to float precision by A.
GAP_RATIO = 4.0
# Measured on an x86-64 host over the committed cases and seeds (tests/triangulate_cases.py), each bound
# 4x the worst value seen.  A wrong rotation formula, sort or transposition errs at the order of 1.
W_MEASURED, W_BOUND = 2.28e-7, 9.2e-7       # max |w - s| / s[0] over the four singular values
V_MEASURED, V_BOUND = 7.78e-7, 3.2e-6       # max |v / |v| -+ v64| over the four components
X_MEASURED, X_BOUND = 8.39e-6, 3.4e-5       # |x3D - x64| / |x64|, OK_TRIANGULATED random pairs
MAX_EXCLUDED_SHARE = 0.05


def _dlt64(c, i1, i2):
    """The linear triangulation in float64 from the float32 inputs."""
    rows = []
    for F, k in ((c["pose1"], c["keys1"][i1]), (c["pose2"], c["keys2"][i2])):
        T = np.concatenate([F["Rcw"].reshape(3, 3).astype(f64), F["tcw"].astype(f64)[:, None]], 1)
        x = (f64(k["x"]) - f64(F["cx"])) / f64(F["fx"])
        y = (f64(k["y"]) - f64(F["cy"])) / f64(F["fy"])
        rows += [x * T[2] - T[0], y * T[2] - T[1]]
    v = np.linalg.svd(np.array(rows))[2][3]
    return v[:3] / v[3]


def test_restated_svd_and_x3d_against_float64():
    worst = dict(w=0.0, v=0.0, x=0.0)
    nrandom = nexcluded = nsvd = 0
    for c in tc.all_cases():
        st, x, infos = tc.reference(c)
        rnd = c["name"].startswith("random")
        for p, info in enumerate(infos):
            if info.get("A") is None:
                continue
            nsvd += 1
            s, vt = np.linalg.svd(info["A"].astype(f64))[1:]
            worst["w"] = max(worst["w"], float(np.abs(info["w"].astype(f64) - s).max() / s[0]))
            excluded = s[3] * GAP_RATIO > s[2]
            nrandom += rnd
            nexcluded += rnd and excluded
            if excluded:
                continue
            v = info["v"].astype(f64)
            v /= np.linalg.norm(v)
            v64 = vt[3] if np.dot(vt[3], v) >= 0 else -vt[3]       # the sign is free
            worst["v"] = max(worst["v"], float(np.abs(v - v64).max()))
            if rnd and st[p] == tc.OK_TRIANGULATED:
                x64 = _dlt64(c, *c["pairs"][p])
                worst["x"] = max(worst["x"], float(np.linalg.norm(x[p].astype(f64) - x64) /
                                                   np.linalg.norm(x64)))
    print(f"restated SVD against float64 on {nsvd} matrices: w {worst['w']:.3g}, "
          f"v {worst['v']:.3g}, x3D {worst['x']:.3g}; {nexcluded} of {nrandom} random excluded")
    assert nsvd > 600 and nrandom > 500
    assert nexcluded <= MAX_EXCLUDED_SHARE * nrandom, (nexcluded, nrandom)
    assert worst["w"] <= W_BOUND and worst["v"] <= V_BOUND and worst["x"] <= X_BOUND, worst
    # the bounds are tight enough to mean something: a wrong decision of the SVD misses them
    c = tc.case_named("near_st00")
    A = tc.reference(c)[2][0]["A"]
    s, vt = np.linalg.svd(A.astype(f64))[1:]
    for bad in (dict(sort_ascending=True),):
        w, Vt = tc.svd_np(A, **bad)
        v = Vt[3].astype(f64) / np.linalg.norm(Vt[3])
        assert min(np.abs(v - vt[3]).max(), np.abs(v + vt[3]).max()) > 1e3 * V_BOUND
