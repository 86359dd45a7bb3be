"""CPU: Sim3Solver as orbx_sim3_* runs it (tests/sim3_cases.py).  The numpy restatement against the
independent cv::Mat restatement of tests/native/sim3_ref.cpp, bit for bit, on every directed and
random case; the census of what the cases contain; every single-decision variant changes a case;
the two host helpers against literal loops; orbx_atan2_f64 against libm; the C ABI's argument
checks, which need no GPU; and a float64 sanity check of the restatement itself."""
import ctypes
import math
import subprocess

import numpy as np
import pytest

import sim3_cases as sc
from my_orb_slam2_amd.features import FRAME_POSE_DTYPE
from my_orb_slam2_amd.sim3 import (RAND_MAX, SIM3_CORR_DTYPE, SIM3_JOB_DTYPE, SIM3_RESULT_DTYPE,
                                   SIM3_STATE_DTYPE, sim3_limits, sim3_ransac_iterations,
                                   sim3_sample_triples)

f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def sim3_ref():
    from my_orb_slam2_amd import build as b
    return b.build_sim3_ref()


@pytest.fixture(scope="module")
def ref_results(sim3_ref, tmp_path_factory):
    d = tmp_path_factory.mktemp("sim3")
    cases = sc.all_cases()
    sc.write_cases(d / "cases.bin", cases)
    subprocess.run([str(sim3_ref), str(d / "cases.bin"), str(d / "out.bin")], check=True,
                   timeout=120)
    return sc.read_results(d / "out.bin", cases)


def test_numpy_equals_cpp_restatement(ref_results):
    """Floats compared as bits; a NaN equals a NaN."""
    for c, per in zip(sc.all_cases(), ref_results):
        r = sc.reference(c)
        assert len(per) == len(r["calls"])
        for k, (call, (rec, inl, st)) in enumerate(zip(r["calls"], per)):
            assert sc.canon(sc.result_record(call).tobytes()) == sc.canon(rec), (c["name"], k)
            assert call["inliers"].tobytes() == inl, (c["name"], k)
            assert tuple(call["state"]) == st, (c["name"], k)


def _events(name):
    return sc.reference(sc.case_named(name))["trace"]


def _holders(pred):
    return {c["name"] for c in sc.all_cases() if not c["name"].startswith("random")
            and any(pred(t) for t in sc.reference(c)["trace"])}


def test_census_exits_events_and_constructs():
    exits = set()
    for c in sc.all_cases():
        exits |= {t["exit"] for t in sc.reference(c)["trace"]}
    assert exits == {"continue", "returned", "max_its", "small_n"}
    # each directed construct is held by the case named for it, and among the directed cases by
    # that case alone
    assert _holders(lambda t: t.get("between_bounds")) == {"between_bounds"}
    assert _holders(lambda t: t.get("at_bound")) == {"at_bound"}
    assert _holders(lambda t: t.get("exit") == "small_n") == {"n_below_min"}
    assert _holders(lambda t: t.get("zero_M")) == {"zero_M_nan"}
    assert _holders(lambda t: t.get("q0_zero")) == {"rotation_180"}
    assert _holders(lambda t: t.get("nonfinite_error")) == {"z_zero"}
    assert _holders(lambda t: t.get("nan_rotation") and not t.get("zero_M")
                    and not t.get("top_pair_equal")) == {"identity_rotation_nan"}
    assert _holders(lambda t: t.get("top_pair_equal") and not t.get("zero_M")) == {"collinear_triple"}
    assert "negative_q0" in _holders(lambda t: t.get("q0_negative"))
    assert "later_tie" in _holders(lambda t: t.get("tie"))
    assert _holders(lambda t: t.get("carried_best")) == {"carried_best_equal", "returned_then_again"}
    assert _holders(lambda t: t.get("exit") == "max_its" and t.get("on_last")
                    ) >= {"max_its_on_last"}
    # the bounds: truncation changes 1.44 * 9.210 and leaves the integer table alone
    assert float(sc.max_error(sc.SIGMA2_12[1])) == 13.0 < 9.210 * float(sc.SIGMA2_12[1])
    for s2 in sc.SIGMA2_INT:
        assert 0 < 9.210 * float(s2) - float(sc.max_error(s2)) < 2e-3
    c = sc.case_named("integer_sigma_table")
    assert sc.reference(c)["calls"][0]["n_inliers"] == 8
    assert sc.key(sc.solve(c, "float_bounds")) == sc.key(sc.reference(c))
    # the count against min_inliers: equal does not return, one above does
    above, equal = (sc.reference(sc.case_named(n)) for n in ("count_above_min", "count_equal_min"))
    assert above["calls"][0]["found"] and above["calls"][0]["n_inliers"] == 7
    assert not equal["calls"][0]["found"] and equal["calls"][0]["state"][1] == 7
    # a carried best: an equal count returns, a lower one does not
    eq = sc.reference(sc.case_named("carried_best_equal"))["calls"]
    lo = sc.reference(sc.case_named("carried_best_lower"))["calls"]
    assert eq[0]["found"] and eq[0]["n_inliers"] == 7 and not any(c["found"] for c in lo)
    # N == min_inliers: one iteration; N < min_inliers: no_more at once, nothing recorded
    ne = sc.reference(sc.case_named("n_equals_min"))
    assert ne["max_its"] == 1 and ne["calls"][0]["state"][0] == 1 and ne["calls"][0]["no_more"]
    nb = sc.reference(sc.case_named("n_below_min"))["calls"][0]
    assert nb["no_more"] and not nb["best_updated"] and nb["state"] == (0, 0)
    # the NaN conventions: all of R12 is NaN and the iteration counts nothing
    for n in ("identity_rotation_nan", "zero_M_nan"):
        call = sc.reference(sc.case_named(n))["calls"][0]
        assert np.isnan(call["model"]["R"]).all() and call["best_inliers"] == 0 and not call["found"]
    # fix_scale
    on, off = (sc.reference(sc.case_named(n))["calls"][0]["model"]["s"]
               for n in ("fix_scale_on", "fix_scale_off"))
    assert on == 1.0 and off != 1.0
    # the draws: the last position, position 0, rand() of 0 and of RAND_MAX
    d = sc.case_named("draw_last_and_zero")
    t = sc.reference(d)["triples"]
    assert t[0].tolist() == [9, 8, 0] and t[1].tolist() == [0, 9, 7]
    assert t[2].tolist() == [0, 9, 8] and t[3].tolist() == [9, 8, 7]
    assert d["rand"][6:12].tolist() == [0] * 3 + [RAND_MAX] * 3
    # i1 sparse and unordered
    i1 = sc.case_named("sparse_i1")["corr"]["i1"]
    assert sc.case_named("sparse_i1")["mN1"] > 2 * len(i1) and (np.diff(i1) < 0).any()
    # the size regimes of the GPU test
    assert {len(c["corr"]) for c in sc.all_cases() if c["name"].startswith("random")} == \
        {3, 4, 19, 20, 21, 63, 64, 65, 129, 300}


@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_every_variant_changes_a_case(variant):
    for c in sorted(sc.all_cases(), key=lambda c: len(c["corr"]) * sum(c["calls"])):
        if sc.key(sc.solve(c, variant)) != sc.key(sc.reference(c)):
            return
    pytest.fail(f"no committed case tells `{variant}` from the restatement")


def test_jacobi_restatement_on_symmetric_matrices():
    """jacobi_eigen against numpy's eigh on random symmetric 4x4 float matrices: the eigenvalues
    descending and each row an eigenvector, to float32 accuracy."""
    rng = np.random.default_rng(3)
    for _ in range(50):
        M = rng.normal(size=(4, 4))
        S = ((M + M.T) / 2).astype(f32)
        W, V, _, _ = sc.jacobi_eigen(S)
        w = np.linalg.eigvalsh(S.astype(f64))[::-1]
        assert (np.diff(W) <= 0).all() and np.abs(W - w).max() < 2e-5
        assert np.abs(V.astype(f64) @ S.astype(f64) - W[:, None].astype(f64) * V).max() < 2e-5
        assert np.abs(V.astype(f64) @ V.T.astype(f64) - np.eye(4)).max() < 1e-5


# ---- the two host helpers ---------------------------------------------------------------------------

def _iterations_literal(prob, min_inliers, max_its, N):
    """:125-135 written out with Python doubles and a float32 quotient."""
    if min_inliers == N:
        n = 1
    else:
        eps = float(f32(min_inliers) / f32(N)) if N else math.inf
        try:
            v = math.ceil(math.log(1 - prob) / math.log(1 - eps ** 3))
        except (ValueError, ZeroDivisionError, OverflowError):
            v = None              # log of a non-positive number, or a quotient by log(1) = 0
        n = v if v is not None and -2 ** 31 <= v < 2 ** 31 else -2 ** 31
    return max(1, min(n, max_its))


def test_ransac_iterations_against_literal_loop(orbx_lib):
    got = {}
    for prob in (0.99, 0.5):
        for N in (20, 21, 40, 100, 1000, 20000, 10 ** 7):
            got[prob, N] = sim3_ransac_iterations(prob, 6, 300, N)
            assert got[prob, N] == _iterations_literal(prob, 6, 300, N) == \
                sc.ransac_iterations_np(prob, 6, 300, N), (prob, N)
    # 6 / 20 as a float: log(0.01) / log(1 - 0.3f^3) = 168.2...
    assert [got[0.99, N] for N in (20, 21, 40, 100, 1000)] == [169, 196, 300, 300, 300]
    assert [got[0.5, N] for N in (20, 21, 40, 100, 1000)] == [26, 30, 206, 300, 300]
    # the quotient is far above INT_MAX, or -inf (pow underflows against 1): INT_MIN, hence 1
    assert got[0.99, 20000] == got[0.99, 10 ** 7] == got[0.5, 20000] == 1
    assert sim3_ransac_iterations(0.99, 6, 300, 6) == 1          # min_inliers == N
    # min_inliers > N: epsilon > 1, the log of a negative number is NaN: INT_MIN, hence 1
    assert sim3_ransac_iterations(0.99, 6, 300, 5) == sc.ransac_iterations_np(0.99, 6, 300, 5) == 1
    assert sim3_ransac_iterations(0.99, 6, 10, 20) == 10         # clipped by max_its
    # the float epsilon and a double one part at the case's probability
    assert sc.ransac_iterations_np(sc.EPS_PROB, sc.EPS_MIN, 300, sc.EPS_N) == 100 == \
        sim3_ransac_iterations(sc.EPS_PROB, sc.EPS_MIN, 300, sc.EPS_N)
    assert sc.ransac_iterations_np(sc.EPS_PROB, sc.EPS_MIN, 300, sc.EPS_N, "double_epsilon") == 101


def test_sample_triples_against_literal_loop(orbx_lib):
    rng = np.random.default_rng(9)
    for N in (3, 4, 5, 19, 64, 300, 8192):
        r = rng.integers(0, RAND_MAX + 1, 3 * 200).astype(np.int32)
        r[:9] = [0, 0, 0, RAND_MAX, RAND_MAX, RAND_MAX, RAND_MAX, 0, RAND_MAX]
        got = sim3_sample_triples(N, r)
        assert np.array_equal(got, sc.sample_triples_np(N, r)), N
        assert ((got >= 0) & (got < N)).all()
        assert (got[:, 0] != got[:, 1]).all() and (got[:, 0] != got[:, 2]).all() and \
            (got[:, 1] != got[:, 2]).all()
    L = orbx_lib
    z = np.zeros(6, np.int32)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert L.orbx_sim3_sample_triples(2, 2, P(z), P(z)) == -1
    assert L.orbx_sim3_sample_triples(5, -1, P(z), P(z)) == -1
    assert L.orbx_sim3_sample_triples(5, 2, None, P(z)) == -1
    assert L.orbx_sim3_sample_triples(5, 2, P(z), None) == -1
    assert L.orbx_sim3_sample_triples(5, 2, P(np.full(6, -1, np.int32)), P(z)) == -1
    assert L.orbx_sim3_sample_triples(5, 0, None, None) == 0


# ---- orbx_atan2_f64 -----------------------------------------------------------------------------------

def _atan2_sample():
    rng = np.random.default_rng(13)
    mag = np.exp(rng.uniform(math.log(1e-12), math.log(1e12), (100000, 2)))
    sign = rng.choice([-1.0, 1.0], (100000, 2))
    pts = [mag * sign]
    sp = [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 2.2e-308, 1e-310,
          1e300, -1e300, 0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** -29, 2.0 ** 66, 2.0 ** 61]
    pts.append(np.array([(a, b) for a in sp for b in sp]))
    # the (norm, w) pairs of the cases: |(x, y, z)| and w of the unit quaternions they produce
    nw = []
    for c in sc.all_cases():
        for t in sc.reference(c)["trace"]:
            if "triple" in t and "rotations" in t:
                nw.append(t["norm_w"])
    pts.append(np.array(nw, f64))
    th = rng.uniform(0, math.pi, 20000)
    pts.append(np.stack([np.sin(th), np.cos(th)], 1))            # unit quaternions of every angle
    return np.concatenate(pts)


def test_atan2_f64_against_libm(sim3_ref, tmp_path):
    """fdlibm documents an error below 1 ulp for atan2 and so does glibc, so the two differ by at
    most 2 ulp; over this sample (every quadrant and magnitude from 1e-12 to 1e12, the axes, signed
    zeros, infinities, NaN, denormals, the interval ends of the reduction, and the (norm, w) pairs
    the cases produce) the measured maximum is 1 ulp.  Special values agree exactly,
    and the numpy transliteration is the same routine bit for bit."""
    yx = _atan2_sample()
    (tmp_path / "in.bin").write_bytes(np.ascontiguousarray(yx, f64).tobytes())
    subprocess.run([str(sim3_ref), "--atan2", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                   check=True, timeout=120)
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), f64).reshape(-1, 2)
    ours, libm = got[:, 0], got[:, 1]
    assert np.array_equal(np.isnan(ours), np.isnan(libm))
    ok = ~np.isnan(libm)
    assert np.array_equal(np.signbit(ours[ok]), np.signbit(libm[ok]))
    with np.errstate(all="ignore"):
        d = np.abs(ours[ok] - libm[ok]) / np.spacing(np.abs(libm[ok]))
    d[ours[ok] == libm[ok]] = 0
    worst = float(d.max())
    print(f"orbx_atan2_f64 against libm on {ok.sum()} pairs: at most {worst:g} ulp apart")
    assert worst <= 2.0
    exact = ~np.isfinite(yx).all(1) | (yx == 0).any(1)
    assert np.array_equal(ours[exact & ok], libm[exact & ok])
    for i in list(range(0, 100000, 97)) + list(range(100000, len(yx))):
        a = sc.atan2_f64(yx[i, 0], yx[i, 1])
        assert f64(a).tobytes() == ours[i].tobytes() or (np.isnan(a) and np.isnan(ours[i])), yx[i]


# ---- the C ABI's argument checks (no GPU needed) ---------------------------------------------------

INVALID, DEVICE, UNSUPPORTED = -1, -2, -4


def _host_args(c):
    r = sc.reference(c)
    pose1 = np.asarray(c["pose1"], FRAME_POSE_DTYPE).reshape(1).copy()
    pose2 = np.asarray(c["pose2"], FRAME_POSE_DTYPE).reshape(1).copy()
    job = sc.job_of(c, r["max_its"], 5).reshape(1).copy()
    tri = np.ascontiguousarray(r["triples"], np.int32)
    state = np.zeros(1, SIM3_STATE_DTYPE)
    res = np.zeros(1, SIM3_RESULT_DTYPE)
    inl = np.full(c["mN1"], 7, np.uint8)
    return dict(pose1=pose1, pose2=pose2, job=job, corr=c["corr"].copy(), tri=tri, state=state,
                res=res, inl=inl)


def test_argument_statuses(orbx_lib):
    import torch
    L = orbx_lib
    lim = sim3_limits()
    assert lim["max_n"] >= 300 and lim["max_its"] >= 300 and lim["max_jobs"] >= 256
    a = _host_args(sc.case_named("count_above_min"))
    P = lambda x: None if x is None else ctypes.c_void_p(x.ctypes.data)

    def host(**kw):
        b = dict(a)
        b.update(kw)
        return L.orbx_sim3_iterate(P(b["pose1"]), P(b["pose2"]), P(b["job"]), P(b["corr"]),
                                   P(b["tri"]), P(b["state"]), P(b["res"]), P(b["inl"]), 0)

    def job(**kw):
        j = a["job"].copy()
        for k, v in kw.items():
            j[k] = v
        return j

    for kw in (dict(pose1=None), dict(pose2=None), dict(job=None), dict(corr=None), dict(tri=None),
               dict(state=None), dict(res=None), dict(inl=None), dict(job=job(N=-1)),
               dict(job=job(mN1=-1)), dict(job=job(n_iterations=-1)), dict(job=job(max_its=0))):
        assert host(**kw) == INVALID, kw
    assert host(job=job(N=lim["max_n"] + 1)) == UNSUPPORTED
    assert host(job=job(max_its=lim["max_its"] + 1)) == UNSUPPORTED
    assert (a["inl"] == 7).all() and not a["res"].tobytes().strip(b"\0")

    def batch(**kw):
        b = dict(m=ctypes.c_void_p(1), jobs=P(a["job"]), njobs=1, max_n=16, max_call=5,
                 poses=P(a["pose1"]), nposes=1, corr=P(a["corr"]), ncorr=len(a["corr"]),
                 tri=P(a["tri"]), ntri=len(a["tri"]), state=P(a["state"]), res=P(a["res"]),
                 inl=P(a["inl"]), ninl=len(a["inl"]))
        b.update(kw)
        return L.orbx_sim3_iterate_batch_device(
            b["m"], b["jobs"], b["njobs"], b["max_n"], b["max_call"], b["poses"], b["nposes"],
            b["corr"], b["ncorr"], b["tri"], b["ntri"], b["state"], b["res"], b["inl"], b["ninl"],
            None)

    # every check below comes before the handle is touched
    for kw in (dict(m=None), dict(njobs=-1), dict(max_n=-1), dict(max_call=-1), dict(nposes=-1),
               dict(ncorr=-1), dict(ntri=-1), dict(ninl=-1), dict(jobs=None), dict(poses=None),
               dict(tri=None), dict(state=None), dict(res=None), dict(corr=None), dict(inl=None)):
        assert batch(**kw) == INVALID, kw
    assert batch(njobs=0) == 0
    assert batch(njobs=lim["max_jobs"] + 1) == UNSUPPORTED
    assert batch(max_n=lim["max_n"] + 1) == UNSUPPORTED
    assert batch(max_call=lim["max_its"] + 1) == UNSUPPORTED
    # within each limit, but the scratch of the three together is above the bound
    assert batch(njobs=lim["max_jobs"], max_n=lim["max_n"], max_call=lim["max_its"]) == UNSUPPORTED
    if not torch.cuda.is_available():
        assert host() == DEVICE


def test_without_gpu_the_host_form_fails_loudly(orbx_lib):
    import torch
    import my_orb_slam2_amd as m
    if torch.cuda.is_available():
        return                      # tests/test_gpu_sim3.py runs the host form where there is one
    c = sc.case_named("count_above_min")
    rand = c["rand"]
    with pytest.raises(m.OrbxError) as e:
        m.Sim3Solver(c["pose1"], c["pose2"], c["corr"], c["sigma2_1"], c["sigma2_2"], c["mN1"],
                     c["fix_scale"], rand).iterate(5)
    assert e.value.code == DEVICE


# ---- the restatement against a float64 Horn solution ---------------------------------------------------

def horn64(P1, P2, fix_scale):
    """Horn 1987 in float64 over numpy's symmetric eigen-solver; P: 3x3, column i = point i."""
    P1, P2 = P1.astype(f64), P2.astype(f64)
    O1, O2 = P1.mean(1, keepdims=True), P2.mean(1, keepdims=True)
    Pr1, Pr2 = P1 - O1, P2 - O2
    M = Pr2 @ Pr1.T
    N = np.array([
        [M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
        [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
        [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
        [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
    N = N + np.triu(N, 1).T
    w, v = np.linalg.eigh(N)
    q = v[:, -1]
    n = np.linalg.norm(q[1:])
    ang = math.atan2(n, q[0])
    R = sc.rodrigues64(2 * ang * q[1:] / n)
    P3 = R @ Pr2
    s = 1.0 if fix_scale else float((Pr1 * P3).sum() / (P3 * P3).sum())
    return R, (O1 - s * R @ O2).reshape(3), s


# The worst deviations measured on the CPU over every iteration of the noiseless directed and
# random cases below (R12 entries, t12 entries in metres at depths of 2.5 to 8 m, s12): 8.8e-7,
# 8.4e-6 and 9.7e-8.  The bounds are four times those; the margin covers float32 conditioning
# the cases do not sample.
HORN_BOUND_R, HORN_BOUND_T, HORN_BOUND_S = 4 * 8.8e-7, 4 * 8.4e-6, 4 * 9.7e-8


def test_restatement_against_float64_horn():
    """On noiseless similarity-transformed points the restated model (float32, OpenCV's forms) is
    compared with a float64 Horn solution of the same triple.  Bounds: four times the worst
    deviation measured over these cases, i.e. 3.5e-6 on the entries of R12, 3.4e-5 m on t12 and
    3.9e-7 on s12.  This checks the restatement, not the kernel."""
    worst = np.zeros(3)
    n = 0
    for seed, N, rot, scale, fix in ((31, 12, (0.1, -0.2, 0.15), 1.1, False),
                                     (32, 20, (1.2, -0.9, 0.8), 0.9, False),
                                     (33, 15, (0.0, 0.0, 3.0), 1.0, True),
                                     (34, 30, (-2.0, 0.5, 0.3), 1.3, False),
                                     (35, 9, (0.01, 0.0, -0.02), 1.0, False)):
        c = sc.make_case("horn", seed, N, rot=rot, scale=scale, fix_scale=fix, max_iterations=12,
                         min_inliers=N, calls=(12,))
        prep, _, _ = sc.prepare(c)
        tri = sc.sample_triples_np(N, c["rand"][:36])
        for t in tri:
            P1 = np.stack([prep[i]["X1"] for i in t], axis=1)
            P2 = np.stack([prep[i]["X2"] for i in t], axis=1)
            # a well-spread minimal set: the solution of a thin triangle is conditioned by it
            d = P2.astype(f64) - P2.astype(f64).mean(1, keepdims=True)
            if np.linalg.svd(d, compute_uv=False)[1] < 0.5:
                continue
            with np.errstate(all="ignore"):
                H = sc.compute_sim3(P1, P2, fix)
            R, tt, s = horn64(P1, P2, fix)
            worst = np.maximum(worst, [np.abs(H["R"] - R).max(), np.abs(H["t"] - tt).max(),
                                       abs(float(H["s"]) - s)])
            n += 1
    print(f"restatement against float64 Horn over {n} triples: R {worst[0]:.3g}, "
          f"t {worst[1]:.3g}, s {worst[2]:.3g}")
    assert n >= 30
    assert worst[0] <= HORN_BOUND_R and worst[1] <= HORN_BOUND_T and worst[2] <= HORN_BOUND_S
