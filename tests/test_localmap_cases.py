"""CPU: Tracking::UpdateLocalMap as orbx_update_local_map* runs it (tests/localmap_cases.py).  The
numpy restatement over the CSR snapshot against the object-level C++ restatement of
tests/native/localmap_ref.cpp (real std::map / std::set over stand-in KeyFrame / MapPoint objects),
integer for integer, on every directed and random case; the census of what the cases contain; every
single-decision variant changes a directed case; the corrupt snapshots are refused; the C ABI's
argument checks and LocalMapView's layout, which need no GPU."""
import ctypes
import subprocess

import numpy as np
import pytest

import localmap_cases as lc

INVALID, DEVICE, UNSUPPORTED = -1, -2, -4


@pytest.fixture(scope="module")
def ref_results(tmp_path_factory):
    from my_orb_slam2_amd import build as b
    exe = b.build_localmap_ref()
    d = tmp_path_factory.mktemp("localmap")
    cases = lc.all_cases()
    lc.write_cases(d / "cases.bin", cases)
    subprocess.run([str(exe), str(d / "cases.bin"), str(d / "out.bin")], check=True, timeout=120)
    return lc.read_results(d / "out.bin", cases)


def test_numpy_equals_cpp_restatement(ref_results):
    """The objects know no capacity: a case the capacities refuse is compared up to the refusal
    by running the restatement again with room."""
    compared = 0
    for c, r in zip(lc.all_cases(), ref_results):
        n = lc.reference(c)
        if n["refused"]:
            assert n["info"] in (lc.CAP_KF, lc.CAP_MP), c["name"]
            n = lc.update_local_map_np(c["S"], dict(c["F"], cap_kf=10 ** 6, cap_mp=10 ** 6))
        assert bool(n["info"] & lc.KEPT) == r["kept"], c["name"]
        assert n["local_kf"] == r["local_kf"], c["name"]
        assert n["ref_kf"] == r["ref_kf"], c["name"]
        assert n["block"][:n["n_local"]] == r["local_mp"], c["name"]
        assert n["nulled"] == r["nulled"], c["name"]
        compared += 1
    assert compared == len(lc.all_cases()) >= 90


def test_census():
    R = lambda name: lc.reference(lc.case_named(name))
    infos = {lc.reference(c)["info"] for c in lc.all_cases()}
    assert {0, lc.KEPT, lc.CAP_KF, lc.CAP_MP} <= infos
    # the tie goes to the first keyframe in kf_order, not the first slot
    assert (R("tie_on_max")["local_kf"], R("tie_on_max")["ref_kf"]) == ([1, 2, 0], 2)
    assert 1 not in R("most_voted_bad")["local_kf"] and R("most_voted_bad")["ref_kf"] == 2
    r = R("all_voted_bad")
    assert (r["info"], r["local_kf"], r["ref_kf"], r["n_local"]) == (0, [], 1, 0) and r["block"]
    for n in ("kept_all_none", "kept_all_outliers", "kept_temporal_only"):
        c = lc.case_named(n)
        r = R(n)
        assert r["info"] == lc.KEPT and r["ref_kf"] == c["F"]["ref_kf"]
        assert r["local_kf"] == list(c["F"]["local_kf"][:c["F"]["n_local_kf"]])
        assert 7 not in r["block"]                       # bad now: rebuilt under the current mp_bad
    assert R("kept_temporal_only")["block"][-2:] == [12, 13]
    # the parent's break: nothing after it
    assert R("parent_missing")["local_kf"] == [0, 1, 2, 4, 3]
    assert R("parent_in_list")["local_kf"] == [0, 1, 2, 4, 3]
    assert R("parent_new_first")["local_kf"] == [0, 1, 2, 5]
    assert R("parent_new_middle")["local_kf"] == [0, 1, 2, 4, 5]
    assert R("parent_new_last")["local_kf"] == [0, 1, 2, 4, 3, 5]
    # the limit of 80
    assert [len(R(f"limit_first_{n}")["local_kf"]) for n in (79, 80, 81, 130)] == [81, 81, 81, 130]
    assert len(R("limit_crossed_mid_loop")["local_kf"]) == 82
    assert R("neighbour_at_10")["local_kf"] == [0, 1, 2, 12]
    assert R("neighbour_at_11")["local_kf"] == [0, 1, 2]
    assert R("neighbour_first_eligible_only")["local_kf"] == [0, 1, 2, 5]
    assert R("neighbour_short_and_empty_rows")["local_kf"] == [0, 1, 2, 3]
    assert R("neighbour_of_an_added_keyframe")["local_kf"] == [0, 1]
    assert R("child_by_kf_order")["local_kf"] == [0, 1, 5]
    assert R("child_bad_skipped")["local_kf"] == [0, 1, 3]
    assert R("child_listed_skipped")["local_kf"] == [0, 1, 2]
    r = R("bad_parent_added")
    assert r["local_kf"] == [0, 2] and r["block"] == [0, 1, 2, 6, 7, 8]
    assert R("points_duplicates_across")["block"] == [0, 1, 2, 3, 4]
    assert R("points_twice_in_one_keyframe")["block"] == [0, 1, 2, 3]
    assert R("points_bad_none_and_empty_keyframe")["block"] == [0, 2, 3]
    r = R("feature_on_bad_point")
    assert r["nulled"] == [0, -1, 3, -1, -1] and r["local_kf"] == [0, 1] and 4 not in r["block"]
    r = R("extras_after_locals")
    assert (r["n_local"], r["block"][6:]) == (6, [10, 7, 9, 6])
    assert r["mp_of_feat"] == [6, 0, 7, 8, 6, 3, 7, 9, -1, 1]
    assert r["skip"] == [1, 1, 0, 1, 0, 0, 1, 1, 1, 1]
    r = R("extras_with_outliers")
    assert r["block"][r["n_local"]:] == [10, 9, 7, 6] and r["mp_of_feat"][2] == -1
    c = lc.case_named("child_row_of_70")
    row = c["S"]["kf_child"][:70]
    first = [k for k, s in enumerate(row) if not c["S"]["kf_bad"][s]][0]
    assert first >= 64 and R("child_row_of_70")["local_kf"] == [0, int(row[first])]
    c = lc.case_named("keyframe_of_2000_features")
    assert c["S"]["kf_mp_off"][1] == 2000 and len(R("keyframe_of_2000_features")["block"]) > 1024
    for n in (1, 64, 65, 130):
        assert len(R(f"n_kf_{n}")["local_kf"]) == n == lc.case_named(f"n_kf_{n}")["F"]["cap_kf"]
    assert len(R("cap_kf_exact")["local_kf"]) == 5 and len(R("cap_mp_exact")["block"]) == 16
    assert R("cap_kf_over_in_extension")["info"] == R("cap_kf_over_in_first_list")["info"] == lc.CAP_KF
    assert R("cap_mp_over")["info"] == R("cap_mp_over_by_the_locals")["info"] == lc.CAP_MP
    # the random cases meet every regime
    rnd = [lc.reference(c) for c in lc.random_cases()]
    assert not any(r["refused"] for r in rnd)
    assert any(r["info"] & lc.KEPT for r in rnd) and any(not r["info"] for r in rnd)
    assert any(len(r["local_kf"]) > 80 for r in rnd)
    assert any(len(r["block"]) > r["n_local"] > 0 for r in rnd)
    assert any(-1 in r["nulled"] and any(m >= 0 for m in r["nulled"]) for r in rnd)


@pytest.mark.parametrize("variant", lc.VARIANTS)
def test_every_variant_changes_a_directed_case(variant):
    changed = [c["name"] for c in lc.directed_cases()
               if lc.result_key(lc.update_local_map_np(c["S"], c["F"], variant)) !=
               lc.result_key(lc.reference(c))]
    assert changed, f"no directed case tells `{variant}` from the restatement"


def test_corrupt_snapshots_are_refused_and_their_healthy_twin_is_not():
    names = set()
    for c in lc.bad_index_cases():
        r = lc.update_local_map_np(c["S"], c["F"])
        assert r["refused"] and r["info"] == lc.BAD_INDEX, c["name"]
        names.add(c["name"])
    # one per array of the view, and the frame's own
    for a in ("kf_order", "kf_parent", "kf_cov_off", "kf_cov", "kf_child_off", "kf_child",
              "kf_mp_off", "kf_mp", "mp_obs_off", "mp_obs", "feat_mp", "nfeat", "kept_list"):
        assert any(n.startswith("bad_" + a) for n in names), a


# ---- LocalMapView.from_lists' layout (no GPU) ---------------------------------------------------------

def test_map_arrays_from_lists_layout():
    from my_orb_slam2_amd.localmap import map_arrays_from_lists
    rec = lc.records(5)
    a = map_arrays_from_lists(
        kf_order=[2, 0, 3, 1], kf_bad=[0, 1, 0, 0], kf_parent=[-1, 0, 0, 0],
        kf_cov=[[1, 2], [], [0], [2, 1, 0]], kf_child=[[1, 2, 3], [], [], []],
        kf_mp=[[0, -1, 1], [], [2, 2], [4]], mp_bad=[0, 0, 1, 0, 0],
        mp_obs=[[0], [0], [2], [], [3]], mp_rec=rec)
    assert a["kf_order"].dtype == np.int32 and a["kf_bad"].dtype == np.uint8
    assert a["kf_cov_off"].tolist() == [0, 2, 2, 3, 6] and a["kf_cov"].tolist() == [1, 2, 0, 2, 1, 0]
    # the children in std::set order: ascending kf_order (slot 1 rank 0, slot 3 rank 1, slot 2 rank 3)
    assert a["kf_child_off"].tolist() == [0, 3, 3, 3, 3] and a["kf_child"].tolist() == [1, 3, 2]
    assert a["kf_mp_off"].tolist() == [0, 3, 3, 5, 6] and a["kf_mp"].tolist() == [0, -1, 1, 2, 2, 4]
    assert a["mp_obs_off"].tolist() == [0, 1, 2, 3, 3, 4] and a["mp_obs"].tolist() == [0, 0, 2, 3]
    assert a["mp_rec"].tobytes() == rec.tobytes() and a["mp_rec"].dtype.itemsize == 32
    # the same snapshot as the case builders make it
    S = lc.snapshot(4, [[0, -1, 1], [], [2, 2], [4]], order=[2, 0, 3, 1], bad_kf=[1],
                    parent=[-1, 0, 0, 0], cov=[[1, 2], [], [0], [2, 1, 0]], bad_mp=[2],
                    obs={3: []}, n_mp=5, rec=rec)
    for k, v in a.items():
        assert np.array_equal(v, S[k]), k
    with pytest.raises(ValueError):
        map_arrays_from_lists([0, 1], [0], [-1, -1], [[], []], [[], []], [[], []], [], [], rec[:0])


# ---- the C ABI's argument checks (no GPU needed) ------------------------------------------------------

def _view_c(S, keep):
    from my_orb_slam2_amd._lib import MapViewC
    c = MapViewC()
    for k in ("n_kf", "n_mp", "n_cov", "n_child", "n_kfmp", "n_obs"):
        setattr(c, k, S[k])
    for k in ("kf_order", "kf_bad", "kf_parent", "kf_cov_off", "kf_cov", "kf_child_off", "kf_child",
              "kf_mp_off", "kf_mp", "mp_bad", "mp_obs_off", "mp_obs", "mp_rec"):
        a = np.ascontiguousarray(S[k])
        keep.append(a)
        setattr(c, k, a.ctypes.data)
    return c


def test_argument_statuses(orbx_lib):
    import torch
    L = orbx_lib
    c = lc.case_named("extras_after_locals")
    S, F = c["S"], c["F"]
    keep = []
    P = lambda a: ctypes.c_void_p(a.ctypes.data)
    n, ck, cm = F["nfeat"], F["cap_kf"], F["cap_mp"]
    bufs = dict(feat=F["feat_mp"].copy(), nfeat=np.array([n], np.int32), lk=np.full(ck, -7, np.int32),
                nlk=np.zeros(1, np.int32), ref=np.full(1, -1, np.int32),
                lmp=np.full(cm, -7, np.int32), nlmp=np.full(2, -7, np.int32),
                mps=np.zeros(cm, lc.MAP_POINT_DTYPE), skip=np.full(cm, 9, np.uint8),
                mpf=np.full(len(F["feat_mp"]), -7, np.int32), info=np.full(1, 77, np.uint32))
    need = L.orbx_update_local_map_scratch_bytes(S["n_kf"], S["n_mp"], 1, ck, cm)
    assert need >= 8 * (S["n_kf"] + S["n_mp"]) and need % 256 == 0
    assert L.orbx_update_local_map_scratch_bytes(S["n_kf"], S["n_mp"], 3, ck, cm) == 3 * need
    assert L.orbx_update_local_map_scratch_bytes(-1, 5, 1, 4, 4) == 0
    scratch = np.zeros(need, np.uint8)
    before = {k: v.copy() for k, v in bufs.items()}

    def batch(view=None, **kw):
        a = dict(view=ctypes.byref(_view_c(S, keep)) if view is None else view, nframes=1,
                 stride=len(F["feat_mp"]), ck=ck, cm=cm, scratch=P(scratch), sb=need)
        a.update({k: P(v) for k, v in bufs.items()})
        a.update(kw)
        return L.orbx_update_local_map_batch_device(
            a["view"], a["nframes"], a["feat"], a["stride"], a["nfeat"], None, a["ck"], a["cm"],
            a["lk"], a["nlk"], a["ref"], a["lmp"], a["nlmp"], a["mps"], a["skip"], a["mpf"],
            a["info"], a["scratch"], a["sb"], None)

    for kw in (dict(nframes=-1), dict(stride=-1), dict(stride=32769), dict(ck=-1), dict(cm=-1),
               dict(sb=need - 1), dict(scratch=None)) + tuple({k: None} for k in bufs):
        assert batch(**kw) == INVALID, kw
    assert batch(view=ctypes.POINTER(type(_view_c(S, keep)))()) == INVALID       # a NULL map
    assert batch(nframes=65536) == UNSUPPORTED
    for field, value, want in (("n_kf", -1, INVALID), ("n_mp", -1, INVALID), ("n_cov", -1, INVALID),
                               ("n_child", -1, INVALID), ("n_kfmp", -1, INVALID),
                               ("n_obs", -1, INVALID), ("n_kf", lc.MAX_KF + 1, UNSUPPORTED),
                               ("kf_order", None, INVALID), ("kf_mp", None, INVALID),
                               ("mp_obs_off", None, INVALID), ("mp_rec", None, INVALID)):
        v = _view_c(S, keep)
        setattr(v, field, value)
        assert batch(view=ctypes.byref(v)) == want, field
    # nothing to do: ORBX_OK with nothing touched, pointers or not
    assert batch(nframes=0) == 0
    assert batch(nframes=0, **{k: None for k in bufs}) == 0

    nlk, ref, info = ctypes.c_int32(0), ctypes.c_int32(-1), ctypes.c_uint32(77)

    def host(view=None, **kw):
        a = dict(view=ctypes.byref(_view_c(S, keep)) if view is None else view, feat=P(bufs["feat"]),
                 n=n, ck=ck, cm=cm, lk=P(bufs["lk"]), nlk=ctypes.byref(nlk), ref=ctypes.byref(ref),
                 lmp=P(bufs["lmp"]), nlmp=P(bufs["nlmp"]), mps=P(bufs["mps"]),
                 skip=P(bufs["skip"]), mpf=P(bufs["mpf"]), info=ctypes.byref(info))
        a.update(kw)
        return L.orbx_update_local_map(a["view"], a["feat"], a["n"], None, a["ck"], a["cm"], a["lk"],
                                       a["nlk"], a["ref"], a["lmp"], a["nlmp"], a["mps"], a["skip"],
                                       a["mpf"], a["info"], 0)

    for kw in (dict(n=-1), dict(n=32769), dict(ck=-1), dict(cm=-1), dict(feat=None), dict(lk=None),
               dict(nlk=None), dict(ref=None), dict(lmp=None), dict(nlmp=None), dict(mps=None),
               dict(skip=None), dict(mpf=None), dict(info=None)):
        assert host(**kw) == INVALID, kw
    v = _view_c(S, keep)
    v.n_kf = lc.MAX_KF + 1
    assert host(view=ctypes.byref(v)) == UNSUPPORTED
    v = _view_c(S, keep)
    v.kf_cov_off = None
    assert host(view=ctypes.byref(v)) == INVALID

    si = L.orbx_local_map_search_inputs_batch_device
    desc = np.zeros((S["n_mp"], 32), np.uint8)
    qd, cl = np.zeros((cm, 32), np.uint8), np.zeros(len(F["feat_mp"]), np.uint8)
    args = lambda: [ctypes.byref(_view_c(S, keep)), P(desc), 1, P(bufs["lmp"]), P(bufs["nlmp"]), cm,
                    P(bufs["mpf"]), len(F["feat_mp"]), P(bufs["nfeat"]), P(qd), P(cl), None]
    for k, bad in ((1, None), (2, -1), (2, 65536), (3, None), (4, None), (5, -1), (6, None), (7, -1),
                   (7, 32769), (8, None), (9, None), (10, None),
                   (1, ctypes.c_void_p(desc.ctypes.data + 1)), (9, ctypes.c_void_p(qd.ctypes.data + 2))):
        a = args()
        a[k] = bad
        assert si(*a) == INVALID, (k, bad)
    a = args()
    a[2] = 0
    assert si(*a) == 0

    for k, v in bufs.items():
        assert v.tobytes() == before[k].tobytes(), k
    assert (nlk.value, ref.value, info.value) == (0, -1, 77)
    if not torch.cuda.is_available():
        assert batch() == DEVICE
        assert host() == DEVICE
        assert si(*args()) == DEVICE


def test_without_gpu_the_host_form_fails_loudly(orbx_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    import my_orb_slam2_amd as m
    c = lc.case_named("extras_after_locals")
    arrays = {k: v for k, v in c["S"].items() if isinstance(v, np.ndarray)}
    with pytest.raises(m.OrbxError) as e:
        m.update_local_map_host(arrays, c["F"]["feat_mp"], c["F"]["cap_kf"], c["F"]["cap_mp"])
    assert e.value.code == DEVICE
