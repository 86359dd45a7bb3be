"""CPU: PnPsolver as orbx_pnp_* runs it (tests/pnp_cases.py).  The Python restatement against the
independent C++ restatement of tests/native/pnp_ref.cpp, bit for bit, on every committed case and
every call of it; the census of what the cases reach; every single-decision variant changes a case;
the restated Jacobi SVD against numpy.linalg.svd and find() against the generating pose; the two
host helpers against the Python text; the C ABI's argument checks, which need no GPU."""
import ctypes
import subprocess

import numpy as np
import pytest

import pnp_cases as pc
from my_orb_slam2_amd.pnp import (PNP_CORR_DTYPE, PNP_JOB_DTYPE, PNP_QR_SINGULAR,
                                  PNP_REFINES_MASK, PNP_RESULT_DTYPE, PNP_STATE_DTYPE,
                                  PNP_SVD_COMPLETED, RAND_MAX, pnp_limits,
                                  pnp_ransac_parameters, pnp_sample_quads, pnp_window)

f32 = np.float32

# 4 x the largest value measured on the CPU over every compute_pose of every committed case
# (DESIGN.md §2): singular values and the residual of the four rows EPnP reads relative to the
# largest singular value; the rotation entries and the translation (m) of find() on exact scenes
SV_BOUND = 7.2e-15
RESIDUAL_BOUND = 8.8e-15
R_BOUND = 1.6e-7
T_BOUND = 1.1e-6


@pytest.fixture(scope="module")
def pnp_ref():
    from my_orb_slam2_amd import build as b
    return b.build_pnp_ref()


@pytest.fixture(scope="module")
def ref_results(pnp_ref, tmp_path_factory):
    d = tmp_path_factory.mktemp("pnp")
    cases = pc.all_cases()
    pc.write_cases(d / "cases.bin", cases)
    subprocess.run([str(pnp_ref), str(d / "cases.bin"), str(d / "out.bin")], check=True, timeout=120)
    return pc.read_results(d / "out.bin", cases)


def test_record_layouts_equal_the_header():
    """sizeof and the offsets that the header's field order and types give (4-byte fields only)."""
    assert PNP_CORR_DTYPE.itemsize == 28 and PNP_CORR_DTYPE.fields["octave"][1] == 24
    assert PNP_JOB_DTYPE.itemsize == 4 * (4 + 16 + 2 + 6 + 3)
    assert [PNP_JOB_DTYPE.fields[k][1] for k in ("sigma2", "nlevels", "th2", "n_matches", "N",
                                                 "corr_off", "inlier_off", "quad_off", "best_off",
                                                 "min_inliers", "max_its", "n_iterations")] == \
        [16, 80, 84, 88, 92, 96, 100, 104, 108, 112, 116, 120]
    assert PNP_STATE_DTYPE.itemsize == 72 and PNP_STATE_DTYPE.fields["best_Tcw"][1] == 8
    assert PNP_RESULT_DTYPE.itemsize == 96
    assert [PNP_RESULT_DTYPE.fields[k][1] for k in ("found", "source", "iteration", "n_run",
                                                    "n_inliers", "no_more", "info",
                                                    "best_inliers", "Tcw")] == \
        [0, 4, 8, 12, 16, 20, 24, 28, 32]


def test_numpy_equals_cpp_restatement(ref_results):
    """Floats compared as bits; a NaN equals a NaN."""
    for c, per in zip(pc.all_cases(), ref_results):
        r = pc.reference(c)
        assert len(per) == len(r["calls"])
        for k, (call, (rec, inl, st, best)) in enumerate(zip(r["calls"], per)):
            assert pc.canon(pc.result_record(call).tobytes()) == pc.canon(rec), (c["name"], k)
            assert pc.expected_inliers(c, call).tobytes() == inl, (c["name"], k)
            assert pc.canon(pc.state_record(call).tobytes()) == pc.canon(st), (c["name"], k)
            assert call["best"].tobytes() == best, (c["name"], k)


def _traces():
    for c in pc.all_cases():
        for k, call in enumerate(pc.reference(c)["calls"]):
            for t in call["trace"]:
                yield c, k, call, t


def _holders(pred):
    return {c["name"] for c, k, call, t in _traces() if pred(c, k, call, t)}


def test_census_exits_and_branches():
    exits = {t["exit"] for _, _, _, t in _traces()}
    assert exits == {"continue", "refined", "best_at_end", "none", "small_n"}
    calls = [(c, k, call) for c in pc.all_cases()
             for k, call in enumerate(pc.reference(c)["calls"])]
    # return through Refine at the first iteration of a solver, and at a later one
    assert any(call["source"] == 1 and call["iteration"] == 1 for _, _, call in calls)
    assert any(call["source"] == 1 and call["iteration"] > 1 and call["n_run"] > 1
               for _, _, call in calls)
    # count >= min whose Refine fails because its count equals min_inliers exactly
    assert "n_equals_min" in _holders(
        lambda c, k, call, t: t.get("refine_count") == pc.reference(c)["min_inliers"]
        and t["exit"] == "continue")
    # the loop-end return of mBestTcw; N == min_inliers with exact data gives it
    ne = pc.reference(pc.case_named("n_equals_min"))
    assert ne["max_its"] == 1 and ne["min_inliers"] == 8 == len(pc.case_named("n_equals_min")["corr"])
    assert ne["calls"][0]["source"] == 2 and ne["calls"][0]["no_more"] == 1
    assert ne["calls"][0]["n_run"] == 5          # `||`: iterate(5) runs five with max_its = 1
    # no model at all; N < min_inliers touches nothing
    nm = pc.reference(pc.case_named("no_model"))["calls"]
    assert not any(c["found"] for c in nm) and all(c["no_more"] for c in nm)
    nb = pc.reference(pc.case_named("n_below_min"))["calls"][0]
    assert nb["no_more"] and nb["n_run"] == 0 and nb["state"][:2] == (0, 0) and nb["inliers"] is None
    # a second call after an early success: window max(max_its - iterations, n), Refine on the
    # carried best set
    ra = pc.reference(pc.case_named("returned_then_again"))
    first, second = ra["calls"][0], ra["calls"][1]
    assert first["found"] and first["iteration"] < ra["max_its"]
    assert pnp_window(ra["max_its"], first["state"][0], 2) == ra["max_its"] - first["state"][0] > 2
    assert any(t.get("carried") for t in second["trace"]) and second["found"]
    # a carried state returned at the loop end without any iteration reaching min_inliers
    cb = pc.reference(pc.case_named("carried_best"))["calls"][0]
    assert cb["source"] == 2 and cb["info"] & PNP_REFINES_MASK == 0
    # every numerical branch, in a hypothesis or in a Refine
    ev = set()
    for _, _, _, t in _traces():
        ev |= t.get("hyp", set()) | t.get("refine", set())
    assert ev >= {"approx_1", "approx_2", "approx_3", "sign_flipped", "sign_kept", "det_negative",
                  "beta_neg", "beta_nonneg", "bksb_skipped", "svd_completed", "qr_singular",
                  "inf_invz", "sort_swapped"}
    assert "equal_z_quad" in _holders(lambda c, k, call, t: "svd_completed" in t.get("hyp", ()))
    assert "identical_quad" in _holders(lambda c, k, call, t: "qr_singular" in t.get("hyp", ()))
    assert "tiny_scene" in _holders(lambda c, k, call, t: "inf_invz" in t.get("hyp", ()))
    # the diagnostics reach the info word
    assert pc.reference(pc.case_named("identical_quad"))["calls"][0]["info"] & PNP_QR_SINGULAR
    assert pc.reference(pc.case_named("equal_z_quad"))["calls"][0]["info"] & PNP_SVD_COMPLETED
    # the sizes of the GPU test
    assert {len(c["corr"]) for c in pc.all_cases()} >= {4, 10, 15, 40, 64, 65, 130}
    assert all(pc.reference(c)["max_its"] <= 35 for c in pc.all_cases())


@pytest.mark.parametrize("variant", pc.VARIANTS)
def test_every_variant_changes_a_case(variant):
    for c in sorted(pc.all_cases(), key=lambda c: len(c["corr"]) * sum(c["calls"])):
        if pc.key(pc.solve(c, variant)) != pc.key(pc.reference(c)):
            return
    pytest.fail(f"no committed case tells `{variant}` from the restatement")


def test_jacobi_restatement_against_numpy_svd():
    """Every 3x3 and 12x12 decomposition of every compute_pose of every case: the singular values,
    and for the 12x12 the residual MtM u - d u and the orthonormality of the four rows EPnP reads,
    all relative to the largest singular value.  A wrong sort, sign or transposition errs at order 1."""
    worst_sv = worst_res = 0.0
    n = 0
    with np.errstate(all="ignore"):
        for c in pc.all_cases():
            for k in pc.svd_records(c):
                for A, w in ((np.array(k["pw0tpw0"]), np.array(k["dc"])),
                             (np.array(k["mtm"]), np.array(k["d"]))):
                    ref = np.linalg.svd(A, compute_uv=False)
                    worst_sv = max(worst_sv, np.abs(w - ref).max() / max(ref[0], 1e-300))
                A = np.array(k["mtm"])
                scale = max(np.linalg.svd(A, compute_uv=False)[0], 1e-300)
                U, d = np.array(k["ut"][8:12]), np.array(k["d"][8:12])
                worst_res = max(worst_res, np.abs(U @ A - d[:, None] * U).max() / scale,
                                np.abs(U @ U.T - np.eye(4)).max())
                n += 1
    print(f"{n} decompositions: singular values {worst_sv:.3e}, residual {worst_res:.3e}")
    assert n > 200
    assert worst_sv <= SV_BOUND and worst_res <= RESIDUAL_BOUND


def test_find_on_exact_scenes_gives_the_generating_pose():
    exact = [c for c in pc.all_cases() if c["exact"]]
    assert {len(c["corr"]) for c in exact} == {10, 15, 40, 64, 65, 130}
    for c in exact:
        f = pc.find(c)
        assert f["found"] and f["n_inliers"] == len(c["corr"]), c["name"]
        T = f["Tcw"].reshape(4, 4).astype(np.float64)
        er, et = np.abs(T[:3, :3] - c["R"]).max(), np.abs(T[:3, 3] - c["t"]).max()
        print(f"{c['name']}: R {er:.3e}, t {et:.3e}")
        assert er <= R_BOUND and et <= T_BOUND, c["name"]
        assert T[3].tolist() == [0, 0, 0, 1]


def test_host_helpers_against_the_python_text(orbx_lib):
    for N in (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 20, 40, 64, 65, 130, 1000, 2048):
        for mi in (4, 8, 10, 15, 50):
            for eps in (0.0, 0.3, 0.4, 0.5, 0.9, 1.0, 1.5):
                for mx in (1, 5, 35, 300):
                    for prob in (0.5, 0.99, 1.0, 0.0):
                        assert pnp_ransac_parameters(prob, mi, mx, 4, eps, N) == \
                            pc.ransac_parameters(prob, mi, mx, 4, eps, N), (N, mi, eps, mx, prob)
    # N == min_inliers: one iteration; Tracking's call (0.99, 10, 300, 4, 0.5, 5.991)
    assert pnp_ransac_parameters(0.99, 10, 300, 4, 0.5, 10) == (10, 1)
    assert pnp_ransac_parameters(0.99, 10, 300, 4, 0.5, 40) == (20, 35)
    assert pnp_ransac_parameters(0.99, 10, 300, 4, 0.5, 0) == (10, 1)
    rng = np.random.default_rng(0)
    for N in (4, 5, 8, 64, 130):
        r = rng.integers(0, RAND_MAX, size=400, endpoint=True).astype(np.int32)
        r[:8] = [0, 0, 0, 0] + [RAND_MAX] * 4
        q = pnp_sample_quads(N, r)
        assert np.array_equal(q, pc.sample_quads(N, r))
        assert all(len(set(row)) == 4 for row in q.tolist()) and q.min() >= 0 and q.max() < N
    assert pnp_sample_quads(4, [0, 0, 0, 0]).tolist() == [[0, 3, 2, 1]]
    lim = pnp_limits()
    assert lim["max_n"] >= 2048 and lim["max_its"] >= 300 and lim["max_jobs"] >= 8


def test_argument_statuses(orbx_lib):
    L = orbx_lib
    a, b = ctypes.c_int32(), ctypes.c_int32()
    assert L.orbx_pnp_ransac_parameters(0.99, 10, 300, 4, 0.5, -1, ctypes.byref(a), ctypes.byref(b)) == -1
    assert L.orbx_pnp_ransac_parameters(0.99, 10, 300, 4, 0.5, 10, None, ctypes.byref(b)) == -1
    assert L.orbx_pnp_ransac_parameters(0.99, 10, 300, 5, 0.5, 10, ctypes.byref(a), ctypes.byref(b)) == -4
    q = np.zeros(4, np.int32)
    r = np.zeros(4, np.int32)
    assert L.orbx_pnp_sample_quads(3, 1, r.ctypes.data, q.ctypes.data) == -1
    assert L.orbx_pnp_sample_quads(4, -1, r.ctypes.data, q.ctypes.data) == -1
    assert L.orbx_pnp_sample_quads(4, 1, None, q.ctypes.data) == -1
    r[2] = -5
    assert L.orbx_pnp_sample_quads(4, 1, r.ctypes.data, q.ctypes.data) == -1
    assert L.orbx_pnp_sample_quads(4, 0, None, None) == 0
    # the batched form: a NULL matcher, and njobs == 0 needs nothing else
    args = [None, None, 0, 0, 0, None, 0, None, 0, None, None, 0, None, None, 0, None]
    assert L.orbx_pnp_iterate_batch_device(*args) == -1
    assert L.orbx_pnp_correspondences_batch_device(None, 0, None, 0, None, 0, None, None, None, 0,
                                                   None, None, None) == -1
    assert L.orbx_pnp_apply_batch_device(None, 0, None, None, None, 0, None, 0, 0, None, None, None,
                                         0, None) == -1
    # the host form: the checks run before the device is touched
    c = pc.case_named("exact_10")
    ref = pc.reference(c)
    job = pc.job_of(c, ref["min_inliers"], ref["max_its"], 5)
    st = np.zeros(1, PNP_STATE_DTYPE)
    best = np.zeros(10, np.uint8)
    res = np.zeros(1, PNP_RESULT_DTYPE)
    inl = np.zeros(c["n_matches"], np.uint8)
    quads = ref["quads"]

    def call(job, corr=c["corr"], quads=quads, st=st, best=best, res=res, inl=inl):
        p = lambda x: None if x is None else x.ctypes.data
        return L.orbx_pnp_iterate(p(job), p(corr), p(quads), p(st), p(best), p(res), p(inl), 0)
    assert call(None) == -1 and call(job, st=None) == -1 and call(job, res=None) == -1
    assert call(job, corr=None) == -1 and call(job, best=None) == -1 and call(job, inl=None) == -1
    assert call(job, quads=None) == -1
    for field, v in (("N", -1), ("n_matches", -1), ("max_its", 0)):
        j = job.copy()
        j[field] = v
        assert call(j) == -1, field
    neg = st.copy()
    neg["iterations"] = -1
    assert call(job, st=neg) == -1
    lim = pnp_limits()
    for field, v in (("N", lim["max_n"] + 1), ("max_its", lim["max_its"] + 1),
                     ("n_iterations", lim["max_its"] + 1)):
        j = job.copy()
        j[field] = v
        assert call(j) == -4, field


def test_without_a_gpu_the_host_form_fails_loudly(orbx_lib):
    import torch
    import my_orb_slam2_amd as m
    if torch.cuda.is_available():
        return                      # tests/test_gpu_pnp.py runs the host form where there is one
    # a solver that iterates, and one below mRansacMinInliers under the class defaults, which has
    # no rand() value to give and still has to reach the entry: both get the device's answer
    below = pc.case_named("n_below_min")
    for s in (pc.solver_of(pc.case_named("exact_10")),
              pc.solver_of(dict(below, corr=below["corr"][:3], rand=np.zeros(0, np.int32)),
                           parameters=False)):
        with pytest.raises(m.OrbxError) as e:
            s.iterate(5)
        assert e.value.code == -2
