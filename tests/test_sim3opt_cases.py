"""CPU: Optimizer::OptimizeSim3 as orbx_sim3_optimize* runs it (tests/sim3opt_cases.py).  The numpy
restatement against the independent C++ restatement of tests/native/sim3opt_ref.cpp, bit for bit,
on every directed and random case; the census of what the cases contain; every single-decision
variant changes a case; orbx_exp_f64 against libm; the exact-observation and planted-outlier cases
against what they were generated from; the C ABI's argument checks, which need no GPU."""
import ctypes
import math
import subprocess

import numpy as np
import pytest

import sim3opt_cases as sc
from my_orb_slam2_amd.features import FRAME_POSE_DTYPE
from my_orb_slam2_amd.sim3 import (SIM3OPT_CORR_DTYPE, SIM3OPT_IN_DTYPE, SIM3OPT_JOB_DTYPE,
                                   SIM3OPT_RESULT_DTYPE)

f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def sim3opt_ref():
    from my_orb_slam2_amd import build as b
    return b.build_sim3opt_ref()


@pytest.fixture(scope="module")
def ref_results(sim3opt_ref, tmp_path_factory):
    d = tmp_path_factory.mktemp("sim3opt")
    cases = sc.all_cases()
    sc.write_cases(d / "cases.bin", cases)
    subprocess.run([str(sim3opt_ref), str(d / "cases.bin"), str(d / "out.bin")], check=True,
                   timeout=120)
    return sc.read_results(d / "out.bin", cases)


def test_record_layouts_match_the_header():
    """The dtypes of sim3.py against the sizes the C structs have (orbx_match.h)."""
    assert SIM3OPT_CORR_DTYPE.itemsize == 4 + 12 + 12 + 8 + 8 + 8
    assert SIM3OPT_JOB_DTYPE.itemsize == 8 + 128 + 8 + 16 + 8
    assert SIM3OPT_IN_DTYPE.itemsize == 52
    assert SIM3OPT_RESULT_DTYPE.itemsize == 16 + 64 + 64
    assert SIM3OPT_RESULT_DTYPE.fields["q"][1] == 16


def test_numpy_equals_cpp_restatement(ref_results):
    """Bitwise: a NaN compares equal to the same NaN."""
    for c, (res, keep) in zip(sc.all_cases(), ref_results):
        r = sc.reference(c)
        what = (c["name"], sc.info_fields(r["res"]["info"]), sc.info_fields(res["info"]))
        assert r["res"].tobytes() == res.tobytes(), what
        assert r["keep"].tobytes() == keep.tobytes(), what


def _kinds(r):
    return {t[3] for t in r["trace"] if len(t) > 3 and isinstance(t[3], str)} | \
           {t[-1] for t in r["trace"] if isinstance(t[-1], str)}


def _branches(r):
    return {t[1:] for t in r["trace"] if t[0] == "exp_branch"}


def test_census_flags_exits_branches_and_counts():
    flags, kinds, branches, more = set(), set(), set(), set()
    counts = set()
    for c in sc.all_cases():
        if c["name"].startswith("random"):
            continue
        r = sc.reference(c)
        f = sc.info_fields(r["res"]["info"])
        flags |= f["flags"]
        kinds |= _kinds(r)
        branches |= _branches(r)
        if f["rounds"] == 2:
            # nMoreIterations: 10 after a dropped pair, 5 otherwise
            more.add(10 if "DROPPED" in f["flags"] else 5)
        if c["name"].startswith("count_"):
            counts.add((len(c["corr"]), c["fix_scale"]))
    assert flags == set(sc.FLAG_NAMES.values()), set(sc.FLAG_NAMES.values()) - flags
    # every exit of the Levenberg loop and of optimize: accepted and rejected trials, the tenth
    # rejection, rho == 0, three small improvements in a row, the iterations running out
    want = {"accept", "reject", "qmax", "rho0", "three_in_a_row", "ran_out"}
    assert want <= kinds, want - kinds
    # Sim3(update): (|sigma| < 1e-5) x (theta < 1e-5)
    assert branches == {(True, True), (True, False), (False, True), (False, False)}
    assert more == {5, 10}
    assert counts == {(n, fs) for n in (0, 1, 9, 10, 11, 63, 64, 65, 129) for fs in (False, True)}
    # ni doubles on rejection: 4, 8, 16 ... in the traces
    nis = {t[4] for c in sc.all_cases() for t in sc.reference(c)["trace"]
           if len(t) == 5 and t[3] == "reject"}
    assert {4.0, 8.0, 16.0, 1024.0, 2048.0} <= nis


def test_census_named_constructs():
    R = lambda n: sc.reference(sc.case_named(n))
    F = lambda n: sc.info_fields(R(n)["res"]["info"])
    # no correspondence: nothing runs; fewer than 10: optimize(5) runs, the call returns 0 with the
    # Sim3 as it came in
    assert F("count_0_free") == dict(rounds=0, iters=0, trials=0, flags={"FEW_INLIERS"})
    for n in ("count_1_free", "count_9_fixed", "nine_left"):
        r, c = R(n), sc.case_named(n)
        assert F(n)["rounds"] == 1 and "FEW_INLIERS" in F(n)["flags"] and r["res"]["n_inliers"] == 0
        start = sc.sim3_from_in(c["sim3_in"])
        assert tuple(r["res"]["q"]) == start[0] and tuple(r["res"]["t"]) == start[1]
        assert float(r["res"]["s"]) == start[2]
    # exactly 10 and exactly 9 pairs left after the first stage
    r = R("ten_left")
    assert r["res"]["n_correspondences"] - r["res"]["n_bad"] == 10 and F("ten_left")["rounds"] == 2
    assert r["res"]["n_inliers"] == 10
    r = R("nine_left")
    assert r["res"]["n_correspondences"] - r["res"]["n_bad"] == 9
    # the dropped pairs stay dropped although the call returned 0
    c = sc.case_named("nine_left")
    assert (r["keep"][c["corr"]["i1"]] == 0).sum() == 5
    # exact observations: chi2 = 0, a zero step through the small branch, rho == 0
    for n in ("exact_free", "exact_fixed"):
        r = R(n)
        assert F(n) == dict(rounds=2, iters=2, trials=2, flags=set())
        assert (r["history"][1][1] == 0).all() and (r["history"][1][2] == 0).all()
        assert "rho0" in _kinds(r) and _branches(r) == {(True, True)}
    assert (False, True) in _branches(R("scale_only"))
    # a pair whose e12 passes while its e21 fails, and the reverse
    bad, c12, c21 = R("outliers_e21_only")["history"][0]
    assert (bad & (c12 <= 10) & (c21 > 10)).any()
    bad, c12, c21 = R("outliers_e12_only")["history"][0]
    assert (bad & (c12 > 10) & (c21 <= 10)).any()
    # chi2 one double ulp on either side of th2 = 10 and on it, in either edge
    for side, col in (("e12", 1), ("e21", 2)):
        for tag, want, dropped in (("below", np.nextafter(10.0, 0), False), ("at", 10.0, False),
                                   ("above", np.nextafter(10.0, 20), True)):
            n = f"chi2_{tag}_th2_{side}"
            h = R(n)["history"][0]
            p = sc.case_named(n)["threshold_pair"]
            assert h[col][p] == want and bool(h[0][p]) == dropped and h[0].sum() == dropped, n
            assert R(n)["res"]["n_inliers"] == 14 - dropped
            # the float comparison would keep all three
            v = sc.optimize_sim3_np(sc.case_named(n), "float_compare")
            assert v["res"]["n_inliers"] == 14
    # a rejected trial that decides the flags
    r = R("rho0_stale")
    v = sc.optimize_sim3_np(sc.case_named("rho0_stale"), "recompute_after_pop")
    assert r["trace"][1:3] == [(0, 0, 1, "reject", 4.0), (0, 0, "terminate", "rho0")]
    assert not np.array_equal(r["history"][0][0], v["history"][0][0])
    # the tenth trial rejected
    assert [t for t in R("count_10_fixed")["trace"] if t[2:] == ("terminate", "qmax")]
    # LDLT::isPositive() false: x keeps the last solution, the trial counts as failed
    for n, rounds in (("nonpositive_11_fixed", 2), ("nonpositive_14_fixed", 2),
                      ("nonpositive_9_free", 1), ("nonpositive_4_fixed", 1)):
        f = F(n)
        assert "NONPOSITIVE_SOLVE" in f["flags"] and f["rounds"] == rounds, (n, f)
        assert f["trials"] > f["iters"]
    # bad geometry runs through: z = 0 gives infinities and NaN, not a special case
    for n in ("z_zero", "z_zero_fixed"):
        h = R(n)["history"][0]
        assert np.isinf(h[2][3]) and h[0][3] and h[0].sum() == 1
    assert R("behind")["res"]["n_bad"] == 1
    # updates outside the limits, finite
    t = [t for t in R("theta_limit")["trace"] if t[0] == "theta_limit"]
    assert t and all(math.isfinite(x[1]) and x[1] > 1048576.0 for x in t)
    t = [t for t in R("exp_limit")["trace"] if t[0] == "exp_limit"]
    assert t and all(math.isfinite(x[1]) and abs(x[1]) > sc.EXP_LIMIT for x in t)
    # octaves 0 and nlevels - 1, nlevels 1 and 16, dense and sparse i1
    assert (sc.case_named("octave_top")["corr"]["octave1"] == sc.NLEVELS - 1).all()
    assert sc.case_named("nlevels_16_top")["corr"]["octave2"].max() == 15
    for n in ("octave_0", "octave_top", "nlevels_16_top", "nlevels_1", "dense_i1", "sparse_i1"):
        assert R(n)["res"]["n_inliers"] == len(sc.case_named(n)["corr"]) > 0
    assert sc.case_named("sparse_i1")["mN1"] == 5000


@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_every_variant_changes_a_case(variant):
    key = lambda r: (r["res"].tobytes(), r["keep"].tobytes())
    # the small cases first: they decide most variants in milliseconds
    for c in sorted(sc.all_cases(), key=lambda c: len(c["corr"])):
        if key(sc.optimize_sim3_np(c, variant)) != key(sc.reference(c)):
            return
    pytest.fail(f"no committed case tells `{variant}` from the restatement")


def test_restated_ldlt_on_definite_and_indefinite_matrices():
    rng = np.random.default_rng(5)
    for k in range(50):
        M = rng.normal(size=(7, 7))
        H = M @ M.T
        b = rng.normal(size=7)
        x = sc.ldlt_solve(H.tolist(), 0.5, b.tolist())
        want = np.linalg.solve(H + 0.5 * np.eye(7), b)
        assert np.allclose(x, want, rtol=1e-9, atol=1e-12)
        D = np.diag(rng.normal(size=7))
        D[k % 7, k % 7] = -abs(D[k % 7, k % 7]) - 0.1
        D[(k + 1) % 7, (k + 1) % 7] = abs(D[(k + 1) % 7, (k + 1) % 7]) + 0.1
        assert sc.ldlt_solve((M @ D @ M.T).tolist(), 0.0, b.tolist()) is None
    assert sc.ldlt_solve(np.zeros((7, 7)).tolist(), 0.0, [1.0] * 7) == [0.0] * 7   # ZeroSign


def test_exp_f64_against_libm(sim3opt_ref, tmp_path):
    """orbx_exp_f64 and libm's exp are both below 1 ulp from the true value, so they differ by at
    most 1 ulp (measured: DESIGN.md §2); exp(0) is exactly 1; the numpy transliteration is the same
    routine bit for bit; outside the limit the routine refuses."""
    rng = np.random.default_rng(12)
    tiny = np.concatenate([10.0 ** rng.uniform(-320, -5, 20000), [5e-324, 2.0 ** -28,
                           np.nextafter(2.0 ** -28, 0), 1e-9, 1e-5, 0.0]])
    x = np.concatenate([rng.uniform(-sc.EXP_LIMIT, sc.EXP_LIMIT, 200000),
                        rng.uniform(-2, 2, 100000), tiny, -tiny,
                        0.5 * math.log(2) * np.arange(-40, 41),          # the reduction's seams
                        np.nextafter(0.5 * math.log(2) * np.arange(-40, 41), 0),
                        [sc.EXP_LIMIT, -sc.EXP_LIMIT, 1.5 * math.log(2), -1.5 * math.log(2)]])
    refused = np.array([np.nextafter(sc.EXP_LIMIT, 1e9), -np.nextafter(sc.EXP_LIMIT, 1e9), np.inf,
                        -np.inf, np.nan])
    (tmp_path / "in.bin").write_bytes(np.concatenate([x, refused]).tobytes())
    subprocess.run([str(sim3opt_ref), "--exp", str(tmp_path / "in.bin"),
                    str(tmp_path / "out.bin")], check=True, timeout=120)
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), f64)
    assert np.isnan(got[-len(refused):]).all()          # refused: the output stays as it was
    got = got[:len(x)]
    want = np.exp(x)
    d = np.abs(got - want) / np.spacing(want)
    worst = float(d.max())
    print(f"orbx_exp_f64 against libm on {len(x)} arguments: at most {worst:g} ulp apart, "
          f"{int((d > 0).sum())} differ")
    assert worst <= 1.0
    assert (got[x == 0.0] == 1.0).all() and (x == 0.0).sum() >= 2
    assert (got[np.abs(x) < 2.0 ** -54] == 1.0).all()
    for i in list(range(0, 3000)) + list(range(len(x) - 200, len(x))):
        assert sc.exp_f64(float(x[i])) == got[i], x[i]
    for v in refused:
        assert sc.exp_f64(float(v)) is None


def test_exact_observations_return_the_generating_sim3():
    for n in ("exact_free", "exact_fixed"):
        c = sc.case_named(n)
        r = sc.reference(c)
        assert tuple(r["res"]["q"]) == (0.0, 0.0, 0.0, 1.0) and float(r["res"]["s"]) == 1.0
        assert (r["res"]["t"] == 0).all()
        assert np.array_equal(r["res"]["T12"].reshape(4, 4), np.eye(4, dtype=f32))
        assert r["res"]["n_inliers"] == len(c["corr"])
        assert r["keep"].tobytes() == c["keep_in"].tobytes()


def test_planted_outliers_and_no_inlier_are_dropped():
    for n in ("outliers_free", "outliers_fixed"):
        c = sc.case_named(n)
        r = sc.reference(c)
        i1 = c["corr"]["i1"]
        assert np.array_equal(r["keep"][i1] == 0, c["planted"]), n
        assert c["planted"].sum() == round(0.3 * len(i1)) == r["res"]["n_bad"]
        assert r["res"]["n_inliers"] == int((~c["planted"]).sum())
        rest = np.ones(c["mN1"], bool)
        rest[i1] = False
        assert (r["keep"][rest] == sc.UNTOUCHED).all() and (r["keep"][i1][~c["planted"]] == 1).all()
        # far from th2 on both sides: the outliers as the first stage saw them, the inliers at the end
        first, last = r["history"]
        assert np.array_equal(first[0], c["planted"]) and not last[0].any()
        assert np.nanmax(np.maximum(last[1], last[2])) < 3.0
        assert np.maximum(first[1], first[2])[c["planted"]].min() > 100 * 10.0
        # and the Sim3 is the generating one.  The scale shows in the images only through the
        # parallax of t12 (0.19 m against 5 m of depth: about 16 px per unit of log s), so 70 pairs
        # with a pixel of noise leave it known to 0.6 %, and t12 along the rays to that share of
        # the depth; the bounds are three such deviations.  The rotation is known to 1e-3 rad.
        R12, t12, s12 = c["gt"]
        Rm = np.array(sc.rotation_matrix(tuple(r["res"]["q"])))
        assert np.abs(Rm - R12).max() < 3e-3
        assert abs(float(r["res"]["s"]) / s12 - 1) < 0.02
        assert np.abs(r["res"]["t"] - t12).max() < 0.1
        if c["fix_scale"]:
            assert float(r["res"]["s"]) == float(c["sim3_in"]["s12"])


def test_result_record_is_consistent():
    for c in sc.all_cases():
        r = sc.reference(c)["res"]
        if not (np.isfinite(r["q"]).all() and np.isfinite(r["t"]).all() and np.isfinite(r["s"])):
            continue
        q = r["q"]
        Rm = np.array(sc.rotation_matrix(tuple(q)))
        T = r["T12"].reshape(4, 4)
        assert np.array_equal(T[:3, :3], (float(r["s"]) * Rm).astype(f32)), c["name"]
        assert np.array_equal(T[:3, 3], r["t"].astype(f32)) and tuple(T[3]) == (0, 0, 0, 1)
        assert abs(np.linalg.norm(q) - 1) < 1e-5, c["name"]      # not normalised, but close


# ---- the C ABI's argument checks (no GPU needed) ---------------------------------------------------

INVALID, DEVICE, UNSUPPORTED = -1, -2, -4


def test_argument_statuses(orbx_lib):
    import torch
    import my_orb_slam2_amd as m
    L = orbx_lib
    c = sc.case_named("count_10_free")
    P = lambda a: ctypes.c_void_p(a.ctypes.data)
    poses = np.stack([np.asarray(c["pose1"], FRAME_POSE_DTYPE).reshape(()),
                      np.asarray(c["pose2"], FRAME_POSE_DTYPE).reshape(())])
    job = sc.job_record(c).reshape(1).copy()
    corr = np.ascontiguousarray(c["corr"])
    sin = np.asarray(c["sim3_in"], SIM3OPT_IN_DTYPE).reshape(1).copy()
    res = np.zeros(1, SIM3OPT_RESULT_DTYPE)
    res["n_inliers"] = -5
    keep = c["keep_in"].copy()
    lim = m.sim3opt_limits()
    assert lim == dict(max_n=4096, max_jobs=65535)

    def host(**kw):
        a = dict(p1=P(poses[0:1]), p2=P(poses[1:2]), job=P(job), corr=P(corr), sin=P(sin),
                 res=P(res), keep=P(keep))
        a.update(kw)
        return L.orbx_sim3_optimize(a["p1"], a["p2"], a["job"], a["corr"], a["sin"], a["res"],
                                    a["keep"], 0)

    for kw in (dict(p1=None), dict(p2=None), dict(job=None), dict(sin=None), dict(res=None),
               dict(corr=None), dict(keep=None)):
        assert host(**kw) == INVALID, kw
    for f, v, want in (("N", -1, INVALID), ("mN1", -1, INVALID),
                       ("N", lim["max_n"] + 1, UNSUPPORTED)):
        j2 = job.copy()
        j2[f] = v
        assert host(job=P(j2)) == want, (f, v)
    assert res["n_inliers"][0] == -5 and keep.tobytes() == c["keep_in"].tobytes()

    matcher = m.ORBmatcher() if torch.cuda.is_available() else None
    h = matcher._h if matcher is not None else ctypes.c_void_p(8)      # only compared with NULL

    def batch(**kw):
        a = dict(m=h, jobs=P(job), njobs=1, max_n=len(corr), poses=P(poses), nposes=2, corr=P(corr),
                 ncorr=len(corr), sin=P(sin), stride=SIM3OPT_IN_DTYPE.itemsize, res=P(res),
                 keep=P(keep), nkeep=len(keep))
        a.update(kw)
        return L.orbx_sim3_optimize_batch_device(
            a["m"], a["jobs"], a["njobs"], a["max_n"], a["poses"], a["nposes"], a["corr"],
            a["ncorr"], a["sin"], a["stride"], a["res"], a["keep"], a["nkeep"], None)

    for kw in (dict(m=None), dict(njobs=-1), dict(max_n=-1), dict(nposes=-1), dict(ncorr=-1),
               dict(nkeep=-1), dict(jobs=None), dict(poses=None), dict(sin=None), dict(res=None),
               dict(corr=None), dict(keep=None), dict(stride=48), dict(stride=54),
               dict(sin=ctypes.c_void_p(sin.ctypes.data + 2))):
        assert batch(**kw) == INVALID, kw
    assert batch(njobs=lim["max_jobs"] + 1) == UNSUPPORTED
    assert batch(max_n=lim["max_n"] + 1) == UNSUPPORTED
    # nothing to do: ORBX_OK with nothing touched, pointers or not
    assert batch(njobs=0) == 0
    assert L.orbx_sim3_optimize_batch_device(h, None, 0, 0, None, 0, None, 0, None, 0, None, None,
                                             0, None) == 0
    assert res["n_inliers"][0] == -5 and keep.tobytes() == c["keep_in"].tobytes()
    if not torch.cuda.is_available():
        assert host() == DEVICE


def test_without_gpu_the_host_form_fails_loudly(orbx_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    import my_orb_slam2_amd as m
    c = sc.case_named("count_10_free")
    with pytest.raises(m.OrbxError) as e:
        m.sim3_optimize(c["pose1"], c["pose2"], sc.job_record(c), c["corr"], c["sim3_in"],
                        c["keep_in"])
    assert e.value.code == DEVICE
    with pytest.raises(m.OrbxError) as e:
        m.OptimizeSim3(c["pose1"], c["pose2"], c["corr"], c["sigma2_1"], c["sigma2_2"], c["mN1"],
                       c["sim3_in"]["R12"], c["sim3_in"]["t12"], float(c["sim3_in"]["s12"]))
    assert e.value.code == DEVICE
