"""CPU: MapPoint::UpdateNormalAndDepth / ComputeDistinctiveDescriptors as orbx_refresh_map_points*
runs them (tests/mprefresh_cases.py).  The numpy restatement against the object-level C++
restatement of tests/native/mprefresh_ref.cpp (a real std::map over stand-in KeyFrame / MapPoint
objects, cv::Mat expressions), bit for bit with NaN components compared as NaN; the census of what
the cases reach; every single-decision variant changes a directed case; the corrupt snapshots are
refused; properties of the results; the C ABI's argument checks, which need no GPU."""
import ctypes
import pathlib
import subprocess

import numpy as np
import pytest

import mprefresh_cases as mc

INVALID, DEVICE, UNSUPPORTED = -1, -2, -4


@pytest.fixture(scope="module")
def ref_results(tmp_path_factory):
    from my_orb_slam2_amd import build as b
    exe = b.build_mprefresh_ref()
    d = tmp_path_factory.mktemp("mprefresh")
    cases = mc.all_cases()
    mc.write_cases(d / "cases.bin", cases)
    subprocess.run([str(exe), str(d / "cases.bin"), str(d / "out.bin")], check=True, timeout=120)
    return mc.read_results(d / "out.bin", cases)


def test_numpy_equals_cpp_restatement(ref_results):
    """The objects know no capacity: the points a max_obs refuses are left out of the comparison
    (the restatement leaves them untouched, which is checked)."""
    compared = nan = 0
    for c, r in zip(mc.all_cases(), ref_results):
        n = mc.reference(c)
        S = c["S"]
        assert not any(w & mc.BAD_INDEX for w in n["info"]), c["name"]
        refused = {int(p) for p, w in zip(c["ids"], n["info"]) if w & mc.REFUSED_ANY}
        for p in refused:
            assert n["rec"][p].tobytes() == S["mp_rec"][p].tobytes(), c["name"]
            assert n["desc"][p].tobytes() == S["mp_desc"][p].tobytes(), c["name"]
        keep = np.array([p not in refused for p in range(S["n_mp"])])
        assert mc.same_records(n["rec"][keep], r["rec"][keep]), c["name"]
        assert n["desc"][keep].tobytes() == r["desc"][keep].tobytes(), c["name"]
        nan += int(np.isnan(n["rec"]["normal"]).any())
        compared += 1
    assert compared == len(mc.all_cases()) >= 40 and nan >= 2


def test_census():
    R = lambda name: mc.reference(mc.case_named(name))
    words = {w for c in mc.all_cases() + mc.bad_index_cases() for w in mc.reference(c)["info"]}
    assert words == {0, mc.SKIPPED_BAD, mc.NO_OBS, mc.DESC_KEPT, mc.CAP_OBS, mc.BAD_INDEX}
    assert R("bad_point")["info"] == [0, mc.SKIPPED_BAD, 0, 0]
    assert R("empty_row")["info"] == [0, mc.NO_OBS, 0]
    assert R("every_keyframe_bad")["info"] == [mc.DESC_KEPT] * 4
    assert R("what_descriptor_all_bad")["info"] == [mc.DESC_KEPT] * 4
    assert R("what_normal_depth_all_bad")["info"] == [0] * 4
    assert R("row_of_256")["info"] == [0, 0] and R("row_of_257")["info"] == [mc.CAP_OBS, 0]
    # one pass and several: the descriptors left after the bad keyframes are dropped
    left = lambda c, p: sum(1 for o in range(c["S"]["mp_obs_off"][p], c["S"]["mp_obs_off"][p + 1])
                            if not c["S"]["kf_bad"][c["S"]["mp_obs"][o]])
    assert left(mc.case_named("64_left_of_80"), 0) == 64
    assert left(mc.case_named("multi_pass_with_bad"), 0) == 100
    assert {left(mc.case_named(f"row_of_{n}"), 0) for n in (63, 64, 65, 128, 256)} == \
        {63, 64, 65, 128, 256}
    # every max_obs class refuses exactly the longer rows
    lens = (1, 3, 4, 32, 33, 64, 65, 100)
    for mo in mc.MAX_OBS_CLASSES:
        assert R(f"max_obs_{mo}")["info"] == [mc.CAP_OBS if n > mo else 0 for n in lens]
    # rank order is not row order there
    c = mc.case_named("rank_order_differs")
    S = c["S"]
    for p in range(2):
        row = S["mp_obs"][S["mp_obs_off"][p]:S["mp_obs_off"][p + 1]]
        ranks = list(S["kf_order"][row])
        assert ranks != sorted(ranks)
    # the absent reference keyframe reads feature 0
    c = mc.case_named("reference_keyframe_absent")
    S = c["S"]
    r = mc.reference(c)
    P = S["kf_pose"][4]
    lvl = S["kf_keys"]["octave"][S["kf_mp_off"][4]]
    d = np.float32(mc._norm_double(S["mp_rec"]["pos"][0] - P["Ow"]))
    assert r["info"][0] == 0 and r["rec"]["max_dist"][0] == d * P["scale"][lvl]
    # the camera centre: NaN in every component, by the copy too
    assert np.isnan(R("point_at_a_camera_centre")["rec"]["normal"][:2]).all()
    assert np.isnan(R("point_at_its_only_camera")["rec"]["normal"][0]).all()
    assert R("point_at_its_only_camera")["rec"]["max_dist"][0] == 0
    assert R("repeated_id")["info"] == [0] * 6
    # the masks write their part alone
    S = mc.case_named("what_normal_depth")["S"]
    r = R("what_normal_depth")
    assert r["desc"].tobytes() == S["mp_desc"].tobytes() and \
        r["rec"].tobytes() != S["mp_rec"].tobytes()
    S = mc.case_named("what_descriptor")["S"]
    r = R("what_descriptor")
    assert r["desc"].tobytes() != S["mp_desc"].tobytes() and \
        r["rec"].tobytes() == S["mp_rec"].tobytes()
    rnd = [mc.reference(c) for c in mc.random_cases()]
    assert {w for r in rnd for w in r["info"]} >= {0, mc.SKIPPED_BAD, mc.NO_OBS}
    assert {c["what"] for c in mc.random_cases()} == {1, 2, 3}
    assert all(c["S"]["n_kf"] <= 40 and c["S"]["n_mp"] <= 300 for c in mc.random_cases())


@pytest.mark.parametrize("variant", mc.VARIANTS)
def test_every_variant_changes_a_directed_case(variant):
    changed = [c["name"] for c in mc.directed_cases()
               if mc.result_key(mc.refresh_np(c["S"], c["ids"], c["what"], c["max_obs"], variant)) !=
               mc.result_key(mc.reference(c))]
    assert changed, f"no directed case tells `{variant}` from the restatement"


def test_corrupt_snapshots_are_refused_and_their_neighbours_are_not():
    causes = set()
    for c in mc.bad_index_cases():
        r = mc.reference(c)
        assert mc.BAD_INDEX in r["info"], c["name"]
        assert set(r["info"]) <= {0, mc.BAD_INDEX}, c["name"]
        assert 0 in r["info"], c["name"]                       # a healthy point beside it
        for p, w in zip(c["ids"], r["info"]):
            if w and 0 <= p < c["S"]["n_mp"]:
                assert r["rec"][p].tobytes() == c["S"]["mp_rec"][p].tobytes(), c["name"]
                assert r["desc"][p].tobytes() == c["S"]["mp_desc"][p].tobytes(), c["name"]
        causes.add(c["cause"])
    assert causes >= {"id_high", "id_negative", "row_decreasing", "row_leaves_mp_obs", "slot_high",
                      "slot_negative", "ref_slot_high", "rank_high", "slot_twice", "rank_twice",
                      "feature_high", "feature_negative", "feature_0_of_an_empty_reference",
                      "nlevels_0", "nlevels_17", "octave_high", "octave_negative"}


def test_result_properties():
    """|normal| <= 1 up to the rounding of n float sums of unit vectors, and the chosen descriptor is
    one of the row's, from a keyframe that is not bad."""
    checked = 0
    for c in mc.all_cases():
        S, r = c["S"], mc.reference(c)
        for p, w in zip(c["ids"], r["info"]):
            if w & ~mc.DESC_KEPT:
                continue
            b, e = S["mp_obs_off"][p], S["mp_obs_off"][p + 1]
            if c["what"] & mc.NORMAL_DEPTH:
                nv = r["rec"]["normal"][p].astype(np.float64)
                if not np.isnan(nv).any():
                    assert np.sqrt((nv * nv).sum()) <= 1 + (e - b + 4) * 2.0 ** -23, c["name"]
                assert r["rec"]["pos"][p].tobytes() == S["mp_rec"]["pos"][p].tobytes()
                assert r["rec"]["min_dist"][p] <= r["rec"]["max_dist"][p]
            if c["what"] & mc.DESCRIPTOR and not w:
                rows = [S["kf_desc"][S["kf_mp_off"][S["mp_obs"][o]] + S["mp_obs_feat"][o]].tobytes()
                        for o in range(b, e) if not S["kf_bad"][S["mp_obs"][o]]]
                assert r["desc"][p].tobytes() in rows, c["name"]
            checked += 1
    assert checked > 500


# ---- the C ABI's argument checks (no GPU needed) ------------------------------------------------------

def _structs(S, keep):
    from my_orb_slam2_amd._lib import MapRefreshC, MapViewC
    v, x = MapViewC(), MapRefreshC()
    for k in ("n_kf", "n_mp", "n_cov", "n_child", "n_kfmp", "n_obs"):
        setattr(v, k, S[k])
    for k in mc.ARRAYS + mc.EXTRA:
        a = np.ascontiguousarray(S[k])
        keep.append(a)
        setattr(x if k in mc.EXTRA else v, k, a.ctypes.data)
    return v, x


def test_argument_statuses(orbx_lib):
    import torch
    L = orbx_lib
    c = mc.case_named("some_keyframes_bad")
    S = c["S"]
    keep = []
    P = lambda a: ctypes.c_void_p(a.ctypes.data)
    ids = c["ids"].copy()
    rec, desc = S["mp_rec"].copy(), S["mp_desc"].copy()
    info = np.full(len(ids), 77, np.uint32)

    def call(fn, vs=None, xs=None, **kw):
        v, x = _structs(S, keep)
        a = dict(view=ctypes.byref(v if vs is None else vs),
                 extra=ctypes.byref(x if xs is None else xs), ids=P(ids),
                 n=len(ids), what=3, max_obs=64, rec=P(rec), desc=P(desc), info=P(info))
        a.update(kw)
        return fn(a["view"], a["extra"], a["ids"], a["n"], a["what"], a["max_obs"], a["rec"],
                  a["desc"], a["info"], None if fn is L.orbx_refresh_map_points_batch_device else 0)

    from my_orb_slam2_amd._lib import MapRefreshC, MapViewC
    for fn in (L.orbx_refresh_map_points_batch_device, L.orbx_refresh_map_points):
        for kw in (dict(n=-1), dict(what=0), dict(what=4), dict(what=7), dict(max_obs=0),
                   dict(max_obs=257), dict(max_obs=-1), dict(ids=None), dict(rec=None),
                   dict(desc=None), dict(info=None)):
            assert call(fn, **kw) == INVALID, (fn.__name__, kw)
        # a NULL map, NULL inputs
        assert call(fn, view=ctypes.POINTER(MapViewC)()) == INVALID
        assert call(fn, extra=ctypes.POINTER(MapRefreshC)()) == INVALID
        for field, value, want in (("n_kf", -1, INVALID), ("n_mp", -1, INVALID),
                                   ("n_kfmp", -1, INVALID), ("n_obs", -1, INVALID),
                                   ("n_kf", 131073, UNSUPPORTED), ("kf_order", None, INVALID),
                                   ("kf_bad", None, INVALID), ("kf_mp_off", None, INVALID),
                                   ("mp_bad", None, INVALID), ("mp_obs_off", None, INVALID),
                                   ("mp_obs", None, INVALID)):
            v, _ = _structs(S, keep)
            setattr(v, field, value)
            assert call(fn, vs=v) == want, (fn.__name__, field)
        for field in mc.EXTRA:
            _, x = _structs(S, keep)
            setattr(x, field, None)
            assert call(fn, xs=x) == INVALID, (fn.__name__, field)
        # the arrays this call does not read may be absent
        v, _ = _structs(S, keep)
        v.kf_parent = v.kf_cov_off = v.kf_cov = v.kf_child_off = v.kf_child = v.kf_mp = v.mp_rec = None
        assert call(fn, vs=v, n=0) == 0
        assert call(fn, n=0) == 0
    # misaligned descriptor arrays, in the device form
    dev = L.orbx_refresh_map_points_batch_device
    _, x = _structs(S, keep)
    x.kf_desc = x.kf_desc + 1
    assert call(dev, xs=x) == INVALID
    assert call(dev, desc=ctypes.c_void_p(desc.ctypes.data + 2)) == INVALID
    assert call(dev, n=0, **{k: None for k in ("ids", "rec", "desc", "info")}) == 0
    assert rec.tobytes() == S["mp_rec"].tobytes() and desc.tobytes() == S["mp_desc"].tobytes()
    assert (info == 77).all()
    if not torch.cuda.is_available():
        assert call(dev) == DEVICE
        assert call(L.orbx_refresh_map_points) == DEVICE


def test_without_gpu_the_host_form_fails_loudly(orbx_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    import my_orb_slam2_amd as m
    c = mc.case_named("some_keyframes_bad")
    S = c["S"]
    with pytest.raises(m.OrbxError) as e:
        m.refresh_map_points_host({k: S[k] for k in mc.ARRAYS}, {k: S[k] for k in mc.EXTRA},
                                  c["ids"], c["what"], 64, S["mp_desc"])
    assert e.value.code == DEVICE


def test_constants_match_the_header():
    from my_orb_slam2_amd import localmap as lm
    assert (lm.REFRESH_NORMAL_DEPTH, lm.REFRESH_DESCRIPTOR) == (mc.NORMAL_DEPTH, mc.DESCRIPTOR)
    assert (lm.REFRESH_SKIPPED_BAD, lm.REFRESH_NO_OBS, lm.REFRESH_DESC_KEPT, lm.REFRESH_CAP_OBS,
            lm.REFRESH_BAD_INDEX, lm.REFRESH_REFUSED_ANY, lm.REFRESH_MAX_OBS) == \
        (mc.SKIPPED_BAD, mc.NO_OBS, mc.DESC_KEPT, mc.CAP_OBS, mc.BAD_INDEX, mc.REFUSED_ANY, mc.MAX_OBS)
    hdr = (pathlib.Path(lm.__file__).resolve().parents[1] / "include" /
           "orbx_localmap.h").read_text()
    for name, v in (("NORMAL_DEPTH 1u", 1), ("DESCRIPTOR 2u", 2), ("SKIPPED_BAD (1u << 0)", 1),
                    ("NO_OBS (1u << 1)", 2), ("DESC_KEPT (1u << 2)", 4), ("CAP_OBS (1u << 8)", 256),
                    ("BAD_INDEX (1u << 10)", 1024), ("MAX_OBS 256", 256)):
        assert "ORBX_REFRESH_" + name in hdr, name
    assert mc.MAP_POINT_DTYPE == lm.MAP_POINT_DTYPE and mc.FRAME_POSE_DTYPE == lm.FRAME_POSE_DTYPE
    assert mc.KEYPOINT_DTYPE == lm.KEYPOINT_DTYPE
