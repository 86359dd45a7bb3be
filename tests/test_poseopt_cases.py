"""CPU: Optimizer::PoseOptimization as orbx_pose_optimization* runs it (tests/poseopt_cases.py).
The numpy restatement against the independent C++ restatement of tests/native/poseopt_ref.cpp, bit
for bit, on every directed and random case; the census of what the cases contain; every
single-decision variant changes a case; orbx_sincos_f64 against libm; the exact-observation and
planted-outlier cases against what they were generated from; the C ABI's argument checks, which
need no GPU."""
import ctypes
import math
import subprocess

import numpy as np
import pytest

import poseopt_cases as pc
from my_orb_slam2_amd.features import FRAME_POSE_DTYPE, MAP_POINT_DTYPE

f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def poseopt_ref():
    from my_orb_slam2_amd import build as b
    return b.build_poseopt_ref()


@pytest.fixture(scope="module")
def ref_results(poseopt_ref, tmp_path_factory):
    d = tmp_path_factory.mktemp("poseopt")
    cases = pc.all_cases()
    pc.write_cases(d / "cases.bin", cases)
    subprocess.run([str(poseopt_ref), str(d / "cases.bin"), str(d / "out.bin")], check=True,
                   timeout=120)
    return pc.read_results(d / "out.bin", cases)


def test_numpy_equals_cpp_restatement(ref_results):
    """Bitwise: a NaN compares equal to the same NaN."""
    for c, (pose, ngood, info, outlier) in zip(pc.all_cases(), ref_results):
        r = pc.reference(c)
        assert r["pose"].tobytes() == pose.tobytes(), c["name"]
        assert r["outlier"].tobytes() == outlier.tobytes(), c["name"]
        assert (r["ngood"], r["info"]) == (ngood, info), (c["name"], pc.info_fields(r["info"]),
                                                         pc.info_fields(info))


def _kinds(r):
    return {t[3] for t in r["trace"] if len(t) > 3 and isinstance(t[3], str)} | \
           {t[-1] for t in r["trace"] if isinstance(t[-1], str)}


def test_census_flags_exits_and_kernel_states():
    flags, kinds, directed_kinds, rounds = set(), set(), set(), set()
    forms = set()
    for c in pc.all_cases():
        r = pc.reference(c)
        f = pc.info_fields(r["info"])
        flags |= f["flags"]
        rounds.add(f["rounds"])
        kinds |= _kinds(r)
        if not c["name"].startswith("random"):
            directed_kinds |= _kinds(r)
        if c["name"].startswith("count_"):
            ur = c["ur"]
            st = np.zeros(len(c["keys"]), bool) if ur is None else ur >= 0
            has = c["mp_of_feat"] >= 0
            forms.add((r["edges"], bool((st & has).any()), bool((~st & has).any())))
    assert flags == set(pc.FLAG_NAMES.values()), flags
    # every exit of the Levenberg loop and of optimize: accepted and rejected trials, the tenth
    # rejection, rho == 0, three small improvements in a row, ten iterations, nothing active
    want = {"accept", "reject", "qmax", "rho0", "three_in_a_row", "ran_out", "empty_optimize",
            "small_theta"}
    assert want <= kinds and want <= directed_kinds, want - directed_kinds
    # both kernel states: four rounds (the last without the kernel) and one round (< 10 edges)
    assert {0, 1, 4} <= rounds
    for ne in (0, 2, 3, 9, 10, 63, 64, 65, 129):
        if ne:
            assert {(ne, False, True), (ne, True, False), (ne, True, True)} <= forms, ne
    # ni doubles on rejection: 4, 8, 16 ... in the traces
    nis = {t[4] for c in pc.all_cases() for t in pc.reference(c)["trace"]
           if len(t) == 5 and t[3] == "reject"}
    assert {4.0, 8.0, 16.0, 1024.0, 2048.0} <= nis


def test_census_named_constructs():
    R = lambda n: pc.reference(pc.case_named(n))
    # exact observations: chi2 = 0, a zero step through the theta < 1e-5 branch, rho == 0
    for n in ("exact_mono", "exact_stereo", "exact_mixed"):
        r = R(n)
        assert pc.info_fields(r["info"]) == dict(rounds=4, iters=4, trials=4, flags=set())
        assert (r["chi2"] == 0).all() and "rho0" in _kinds(r) and ("small_theta",) in r["trace"]
    assert ("small_theta",) in R("start_at_optimum")["trace"]
    # the tenth trial rejected: the classification reads the errors of that popped trial, every
    # edge's chi2 differs from the one recomputed at the restored estimate (by 1e-11 relative here:
    # the tenth step is 2^-55 of the first; no committed frame turns that into a flipped flag)
    r = R("count_65_stereo")
    assert [t for t in r["trace"] if t[0] == 0 and t[2:] == ("terminate", "qmax")]
    v = pc.pose_optimization_np(pc.case_named("count_65_stereo"), "recompute_after_pop")
    assert (r["history"][0][1] != v["history"][0][1]).all()
    assert np.allclose(r["history"][0][1], v["history"][0][1], rtol=1e-9, atol=0)
    # a popped trial that does decide the flags
    r, v = R("rho0_stale"), pc.pose_optimization_np(pc.case_named("rho0_stale"), "recompute_after_pop")
    assert r["trace"][:2] == [(0, 0, 1, "reject", 4.0), (0, 0, "terminate", "rho0")]
    assert r["ngood"] == 13 and v["ngood"] == 0
    assert "three_in_a_row" in _kinds(R("slow_0"))
    # an outlier after round 0 that is an inlier at the end
    h = R("slow_3")["history"]
    assert (h[0][0] & ~h[3][0]).any()
    # the result changes when the kernel is kept after round 2
    key = lambda r: (r["pose"].tobytes(), r["outlier"].tobytes(), r["ngood"], r["info"])
    c = pc.case_named("borderline_0")
    assert key(pc.pose_optimization_np(c, "kernel_kept")) != key(R("borderline_0"))
    # every edge an outlier after round 0
    r = R("far_3_mono")
    assert r["history"][0][0].all() and [t for t in r["trace"] if t[1:] == ("empty_optimize",)]
    # one float ulp around 5.991f
    for n, want in (("chi2_at_threshold", f32(5.991)),
                    ("chi2_above_threshold", np.nextafter(f32(5.991), f32(9)))):
        c = pc.case_named(n)
        e = int(np.flatnonzero(np.flatnonzero(c["mp_of_feat"] >= 0) == c["threshold_feat"])[0])
        bad, chi2 = R(n)["history"][1]
        assert f32(chi2[e]) == want and chi2[e] > float(f32(5.991))
        assert bool(bad[e]) == (n == "chi2_above_threshold")
    # LDLT::isPositive() false: x keeps the last solution, the trial counts as failed; in one
    # round and in four, mono, stereo and interleaved, ending on rho == 0 and on the tenth trial
    for n, rounds in (("nonpositive_mono_5", 1), ("nonpositive_mono_3", 1),
                      ("nonpositive_stereo_14", 4), ("nonpositive_stereo_4_qmax", 1),
                      ("nonpositive_mixed_11", 4)):
        f = pc.info_fields(R(n)["info"])
        assert f["flags"] == {"NONPOSITIVE_SOLVE"} and f["rounds"] == rounds, (n, f)
        assert f["trials"] > f["iters"]
    assert "qmax" in _kinds(R("nonpositive_stereo_4_qmax"))
    # bad geometry runs through: z = 0 gives infinities, not a special case
    assert "THETA_LIMIT" in pc.info_fields(R("z_zero")["info"])["flags"]
    assert R("behind")["ngood"] == 19
    t = [t for t in R("theta_limit")["trace"] if t[0] == "theta_limit"]
    assert t and all(math.isfinite(x[1]) and x[1] > pc.SINCOS_LIMIT for x in t)
    # octaves 0 and nlevels - 1, nlevels 1 and 16
    assert (pc.case_named("octave_top")["keys"]["octave"] == pc.NLEVELS - 1).all()
    assert pc.case_named("nlevels_16_top")["keys"]["octave"].max() == 15
    for n in ("octave_0", "octave_top", "nlevels_16_top", "nlevels_1", "octave_unread"):
        assert R(n)["ngood"] == R(n)["edges"] > 0


@pytest.mark.parametrize("variant", pc.VARIANTS)
def test_every_variant_changes_a_case(variant):
    key = lambda r: (r["pose"].tobytes(), r["outlier"].tobytes(), r["ngood"], r["info"])
    # the small cases first: they decide most variants in milliseconds
    for c in sorted(pc.all_cases(), key=lambda c: len(c["keys"])):
        if key(pc.pose_optimization_np(c, variant)) != key(pc.reference(c)):
            return
    pytest.fail(f"no committed case tells `{variant}` from the restatement")


def test_restated_ldlt_on_definite_and_indefinite_matrices():
    rng = np.random.default_rng(5)
    for k in range(50):
        M = rng.normal(size=(6, 6))
        H = M @ M.T
        b = rng.normal(size=6)
        x = pc.ldlt_solve(H.tolist(), 0.5, b.tolist())
        want = np.linalg.solve(H + 0.5 * np.eye(6), b)
        assert np.allclose(x, want, rtol=1e-9, atol=1e-12)
        D = np.diag(rng.normal(size=6))
        D[k % 6, k % 6] = -abs(D[k % 6, k % 6]) - 0.1
        D[(k + 1) % 6, (k + 1) % 6] = abs(D[(k + 1) % 6, (k + 1) % 6]) + 0.1
        assert pc.ldlt_solve((M @ D @ M.T).tolist(), 0.0, b.tolist()) is None
    assert pc.ldlt_solve(np.zeros((6, 6)).tolist(), 0.0, [1.0] * 6) == [0.0] * 6   # ZeroSign


def test_sincos_f64_against_libm(poseopt_ref, tmp_path):
    """orbx_sincos_f64 and libm's sin / cos are both below 1 ulp from the true value, so they
    differ by at most 1 ulp (measured: DESIGN.md §2); the numpy transliteration is the same
    routine bit for bit; outside the limit the routine refuses."""
    rng = np.random.default_rng(11)
    x = np.concatenate([np.exp(rng.uniform(math.log(1e-5), math.log(pc.SINCOS_LIMIT), 200000)),
                        np.arange(1, 4001) * (math.pi / 2),            # next to the zeros
                        np.nextafter(np.arange(1, 4001) * (math.pi / 2), 0),
                        [1e-5, pc.SINCOS_LIMIT, math.pi / 4, np.nextafter(math.pi / 4, 1)]])
    x = x[x <= pc.SINCOS_LIMIT]
    (tmp_path / "in.bin").write_bytes(np.concatenate([x, [np.nextafter(pc.SINCOS_LIMIT, 1e9),
                                                          np.inf, np.nan]]).tobytes())
    subprocess.run([str(poseopt_ref), "--sincos", str(tmp_path / "in.bin"),
                    str(tmp_path / "out.bin")], check=True, timeout=120)
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), f64).reshape(-1, 2)
    assert np.isnan(got[-3:]).all()                     # refused: the outputs stay as they were
    got = got[:-3]
    worst = 0.0
    for col, fn in ((0, np.sin), (1, np.cos)):
        want = fn(x)
        ulp = np.spacing(np.abs(want))
        d = np.abs(got[:, col] - want) / ulp
        worst = max(worst, float(d.max()))
    print(f"orbx_sincos_f64 against libm on {len(x)} arguments: at most {worst:g} ulp apart")
    assert worst <= 1.0
    for v in list(x[:2000]) + list(x[-8005:]):
        assert pc.sincos_f64(float(v)) == tuple(got[np.flatnonzero(x == v)[0]])
    assert pc.sincos_f64(float(np.nextafter(pc.SINCOS_LIMIT, 1e9))) is None
    assert pc.sincos_f64(float("nan")) is None


def test_exact_observations_return_the_generating_pose():
    for n in ("exact_mono", "exact_stereo", "exact_mixed"):
        c = pc.case_named(n)
        r = pc.reference(c)
        Rgt, tgt = c["gt"]
        assert r["pose"]["Rcw"].tobytes() == Rgt.reshape(9).tobytes()
        assert r["pose"]["tcw"].tobytes() == tgt.tobytes()
        assert (r["pose"]["Ow"] == 0).all()
        assert r["ngood"] == r["edges"] and not r["outlier"][c["mp_of_feat"] >= 0].any()


def test_planted_outliers_and_no_inlier_are_flagged():
    for n in ("outliers_mono", "outliers_stereo", "outliers_mixed"):
        c = pc.case_named(n)
        r = pc.reference(c)
        has = c["mp_of_feat"] >= 0
        assert np.array_equal(r["outlier"][has] == 1, c["planted"][has]), n
        assert (r["outlier"][~has] == pc.UNTOUCHED).all()
        assert r["ngood"] == int((~c["planted"][has]).sum())
        assert c["planted"][has].sum() == round(0.3 * has.sum())
        # far from the thresholds on both sides
        assert r["chi2"][~c["planted"][has]].max() < 3.0
        assert r["chi2"][c["planted"][has]].min() > 100 * 7.815
        # and the pose is the generating one to a fraction of a pixel at 5 m
        Rgt, tgt = c["gt"]
        assert np.abs(r["pose"]["Rcw"] - Rgt.reshape(9)).max() < 2e-3
        assert np.abs(r["pose"]["tcw"] - tgt).max() < 2e-2


def test_output_pose_is_a_rotation_and_ow_its_centre():
    for c in pc.all_cases():
        r = pc.reference(c)
        if pc.info_fields(r["info"])["rounds"] == 0:      # refused or too few edges: copied through
            assert r["pose"].tobytes() == np.asarray(c["pose"]).tobytes()
            continue
        if not (np.isfinite(r["pose"]["Rcw"]).all() and np.isfinite(r["pose"]["tcw"]).all()):
            continue
        Rm = r["pose"]["Rcw"].reshape(3, 3).astype(f64)
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-6, c["name"]
        ow = -(Rm.T @ r["pose"]["tcw"].astype(f64))
        assert np.allclose(r["pose"]["Ow"], ow, rtol=1e-5, atol=1e-5 * (1 + np.abs(ow).max()))
        for k in ("fx", "fy", "cx", "cy", "mbf", "nlevels", "scale", "min_x", "log_scale_factor"):
            assert np.array_equal(r["pose"][k], c["pose"][k])


# ---- the C ABI's argument checks (no GPU needed) ---------------------------------------------------

INVALID, DEVICE = -1, -2


def test_argument_statuses(orbx_lib):
    import torch
    L = orbx_lib
    c = pc.case_named("count_10_mixed")
    P = lambda a: ctypes.c_void_p(a.ctypes.data)
    pose = np.asarray(c["pose"], FRAME_POSE_DTYPE).reshape(1).copy()
    keys, ur, mpf = c["keys"].copy(), c["ur"].copy(), c["mp_of_feat"].copy()
    mps = np.ascontiguousarray(c["mps"], MAP_POINT_DTYPE)
    n, nmp = len(keys), len(mps)
    out = np.zeros(1, FRAME_POSE_DTYPE)
    flag = c["outlier_in"].copy()
    ngood, info = ctypes.c_int32(-5), ctypes.c_uint32(77)

    def host(**kw):
        a = dict(pose=P(pose), keys=P(keys), ur=P(ur), n=n, mpf=P(mpf), mps=P(mps), nmp=nmp,
                 out=P(out), flag=P(flag), ngood=ctypes.byref(ngood), info=ctypes.byref(info))
        a.update(kw)
        return L.orbx_pose_optimization(a["pose"], a["keys"], a["ur"], a["n"], a["mpf"], a["mps"],
                                        a["nmp"], a["out"], a["flag"], a["ngood"], a["info"], 0)

    for kw in (dict(pose=None), dict(out=None), dict(ngood=None), dict(n=-1), dict(n=32769),
               dict(nmp=-1), dict(keys=None), dict(mpf=None), dict(flag=None), dict(mps=None)):
        assert host(**kw) == INVALID, kw
    assert (ngood.value, info.value) == (-5, 77) and flag.tobytes() == c["outlier_in"].tobytes()

    off = np.array([0, n], np.int32)
    moff = np.array([0, nmp], np.int32)
    ng, inf = np.full(1, -5, np.int32), np.full(1, 77, np.uint32)

    def batch(**kw):
        a = dict(poses=P(pose), nframes=1, keys=P(keys), ur=P(ur), off=P(off), max_feat=n,
                 mpf=P(mpf), mps=P(mps), moff=P(moff), out=P(out), flag=P(flag), ng=P(ng),
                 inf=P(inf))
        a.update(kw)
        return L.orbx_pose_optimization_batch_device(
            a["poses"], a["nframes"], a["keys"], a["ur"], a["off"], a["max_feat"], a["mpf"],
            a["mps"], a["moff"], a["out"], a["flag"], a["ng"], a["inf"], None)

    for kw in (dict(nframes=-1), dict(nframes=65536), dict(max_feat=-1), dict(max_feat=32769),
               dict(poses=None), dict(keys=None), dict(off=None), dict(mpf=None), dict(mps=None),
               dict(moff=None), dict(out=None), dict(flag=None), dict(ng=None), dict(inf=None)):
        assert batch(**kw) == INVALID, kw
    # nothing to do: ORBX_OK with nothing touched, pointers or not
    assert batch(nframes=0) == 0
    assert L.orbx_pose_optimization_batch_device(None, 0, None, None, None, 0, None, None, None,
                                                 None, None, None, None, None) == 0
    assert (ng[0], inf[0]) == (-5, 77)

    m2f = L.orbx_matches_to_features_batch_device
    z = np.zeros(4, np.int32)
    assert m2f(P(z), P(z), P(z), -1, 4, 4, None, P(z), P(z), None) == INVALID
    assert m2f(P(z), P(z), P(z), 65536, 4, 4, None, P(z), P(z), None) == INVALID
    assert m2f(P(z), P(z), P(z), 1, -1, 4, None, P(z), P(z), None) == INVALID
    assert m2f(P(z), P(z), P(z), 1, 4, 32769, None, P(z), P(z), None) == INVALID
    for k in (0, 1, 2, 7, 8):
        a = [P(z), P(z), P(z), 1, 4, 4, None, P(z), P(z), None]
        a[k] = None
        assert m2f(*a) == INVALID, k
    assert m2f(None, None, None, 0, 0, 0, None, None, None, None) == 0
    if not torch.cuda.is_available():
        assert host() == DEVICE
        assert batch() == DEVICE
        assert m2f(P(z), P(z), P(z), 1, 4, 4, None, P(z), P(z), None) == DEVICE


def test_without_gpu_the_host_form_fails_loudly(orbx_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    import my_orb_slam2_amd as m
    c = pc.case_named("count_10_mixed")
    with pytest.raises(m.OrbxError) as e:
        m.pose_optimization(c["pose"], c["keys"], c["mp_of_feat"], c["mps"], c["ur"])
    assert e.value.code == DEVICE
