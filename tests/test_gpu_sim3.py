"""GPU: orbx_sim3_iterate / orbx_sim3_iterate_batch_device (k_sim3_prepare, k_sim3_hypotheses,
k_sim3_select) bit for bit against the numpy restatement of tests/sim3_cases.py (which
tests/test_sim3_cases.py holds against the C++ restatement on the CPU), with sentinels in and
around every output; refused jobs beside good ones; the limits; and the chain SearchByBoW(KF, KF)
-> Sim3Solver -> SIM3 projection -> SearchBySim3 against the oracle fed by the restatement."""
import ctypes

import numpy as np
import pytest

import projection_cases as pc
import sim3_cases as sc
from my_orb_slam2_amd import synth
from my_orb_slam2_amd._lib import check, ptr
from my_orb_slam2_amd.features import (FRAME_POSE_DTYPE, PROJ_SIM3, frame_pose, proj_job,
                                       project_map_points)
from my_orb_slam2_amd.sim3 import (SIM3_CORR_DTYPE, SIM3_JOB_DTYPE, SIM3_REFUSED_I1,
                                   SIM3_REFUSED_LIMIT, SIM3_REFUSED_OCTAVE, SIM3_REFUSED_RANGE,
                                   SIM3_REFUSED_TRIPLE, SIM3_RESULT_DTYPE, SIM3_STATE_DTYPE,
                                   Sim3Solver, sim3_iterate, sim3_limits, sim3_ransac_iterations,
                                   sim3_sample_triples)

pytestmark = pytest.mark.gpu
S = sc.SENTINEL
GUARD = 64                      # sentinel bytes between the jobs' inlier blocks


def _sentinel(n, dtype):
    return np.frombuffer(bytes([S]) * (n * dtype.itemsize), dtype).copy()


def _setup(case):
    """max_its and the triples through the library's own helpers."""
    N = len(case["corr"])
    r = sc.reference(case)
    max_its = sim3_ransac_iterations(case["prob"], case["min_inliers"], case["max_iterations"], N)
    assert max_its == r["max_its"]
    tri = sim3_sample_triples(N, case["rand"][:3 * max_its]) if N >= 3 else \
        np.zeros((max_its, 3), np.int32)
    assert np.array_equal(tri, r["triples"])
    return r, max_its, tri


def test_host_form_every_case(orbx_lib, gpu):
    for c in sc.all_cases():
        r, max_its, tri = _setup(c)
        state = np.zeros(1, SIM3_STATE_DTYPE)
        state["iterations"], state["best_inliers"] = c["state0"]
        for k, (n_it, call) in enumerate(zip(c["calls"], r["calls"])):
            res, inl = _sentinel(1, SIM3_RESULT_DTYPE), _sentinel(c["mN1"], np.dtype(np.uint8))
            sim3_iterate(c["pose1"], c["pose2"], sc.job_of(c, max_its, n_it), c["corr"], tri,
                         state, res, inl)
            assert sc.canon(res.tobytes()) == sc.canon(sc.result_record(call).tobytes()), \
                (c["name"], k, res, sc.result_record(call))
            assert inl.tobytes() == call["inliers"].tobytes(), (c["name"], k)
            assert (int(state["iterations"][0]), int(state["best_inliers"][0])) == call["state"]


class Batch:
    """The device arrays of one batched call over `items` = [(case, max_its, triples)], each job
    with its own slice of every array and sentinels between and around them."""

    def __init__(self, items, gpu):
        import torch
        self.items, self.gpu, self.torch = items, gpu, torch
        self.n = len(items)
        self.poses = np.concatenate([np.stack([np.asarray(c["pose1"], FRAME_POSE_DTYPE).reshape(()),
                                               np.asarray(c["pose2"], FRAME_POSE_DTYPE).reshape(())])
                                     for c, _, _ in items])
        self.corr = np.concatenate([c["corr"] for c, _, _ in items] +
                                   [np.zeros(1, SIM3_CORR_DTYPE)])
        self.tri = np.concatenate([t.reshape(-1, 3) for _, _, t in items]).astype(np.int32)
        self.corr_off = np.cumsum([0] + [len(c["corr"]) for c, _, _ in items])
        self.tri_off = np.cumsum([0] + [len(t) for _, _, t in items])
        self.inl_off = np.cumsum([GUARD] + [c["mN1"] + GUARD for c, _, _ in items])
        self.state = _sentinel(self.n + 2, SIM3_STATE_DTYPE)
        for j, (c, _, _) in enumerate(items):
            self.state[j + 1] = c["state0"]

    def dev(self, a):
        return self.torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).to(self.gpu)

    def call(self, matcher, n_iterations, max_n=None, max_call=None, edit=None):
        """One iterate(n_iterations[j]) of every job -> (results, inlier bytes, states)."""
        jobs = np.zeros(self.n, SIM3_JOB_DTYPE)
        windows = []
        for j, (c, max_its, _) in enumerate(self.items):
            jobs[j] = sc.job_of(c, max_its, n_iterations[j], kf1=2 * j, kf2=2 * j + 1,
                                corr_off=self.corr_off[j], inlier_off=self.inl_off[j],
                                triple_off=self.tri_off[j])
            windows.append(max(0, min(max_its - int(self.state[j + 1]["iterations"]),
                                      n_iterations[j])))
        corr, tri = self.corr, self.tri
        if edit:
            jobs, corr, tri = edit(jobs, corr.copy(), tri.copy())
        max_n = max(len(c["corr"]) for c, _, _ in self.items) if max_n is None else max_n
        max_call = max(windows) if max_call is None else max_call
        res = _sentinel(self.n + 2, SIM3_RESULT_DTYPE)
        inl = np.full(int(self.inl_off[-1]), S, np.uint8)
        d = [self.dev(a) for a in (jobs, self.poses, corr, tri, self.state[1:-1], res, inl)]
        d_state = self.dev(self.state)
        d_res = d[5]
        item = SIM3_RESULT_DTYPE.itemsize
        matcher.sim3_iterate_batch_device(
            d[0], self.n, max_n, max_call, d[1], d[2], d[3],
            d_state[SIM3_STATE_DTYPE.itemsize:-SIM3_STATE_DTYPE.itemsize],
            d_res[item:-item], d[6])
        matcher.sync()
        res = np.frombuffer(d_res.cpu().numpy().tobytes(), SIM3_RESULT_DTYPE)
        inl = d[6].cpu().numpy()
        state = np.frombuffer(d_state.cpu().numpy().tobytes(), SIM3_STATE_DTYPE).copy()
        # the guards around the results and the states, and between the inlier blocks
        assert res[[0, -1]].tobytes() == bytes([S]) * (2 * item)
        assert state[[0, -1]].tobytes() == bytes([S]) * 16
        for j in range(self.n + 1):
            assert (inl[self.inl_off[j] - GUARD:self.inl_off[j]] == S).all()
        self.state = state
        return res[1:-1], [inl[self.inl_off[j]:self.inl_off[j] + c["mN1"]]
                           for j, (c, _, _) in enumerate(self.items)], state[1:-1]


@pytest.fixture(scope="module")
def matcher(orbx_lib, gpu):
    from my_orb_slam2_amd import ORBmatcher
    m = ORBmatcher(0.75, True)
    if not hasattr(m, "sync"):
        m.sync = lambda: check("orbx_matcher_sync", m._lib.orbx_matcher_sync(m._h, None))
    return m


def _run_group(matcher, gpu, cases):
    items = [(c,) + _setup(c)[1:] for c in cases]
    refs = [sc.reference(c)["calls"] for c in cases]
    b = Batch(items, gpu)
    for k in range(max(len(c["calls"]) for c in cases)):
        # a job whose case has no k-th call repeats iterate(0): nothing but no_more may change
        n_it = [c["calls"][k] if k < len(c["calls"]) else 0 for c in cases]
        before = b.state[1:-1].copy()
        res, inl, state = b.call(matcher, n_it)
        for j, c in enumerate(cases):
            if k >= len(c["calls"]):
                assert state[j] == before[j] and not res[j]["found"] and not res[j]["best_updated"]
                continue
            call = refs[j][k]
            assert sc.canon(res[j:j + 1].tobytes()) == sc.canon(sc.result_record(call).tobytes()), \
                (c["name"], k, res[j], sc.result_record(call))
            assert inl[j].tobytes() == call["inliers"].tobytes(), (c["name"], k)
            assert (int(state[j]["iterations"]), int(state[j]["best_inliers"])) == call["state"]


@pytest.mark.parametrize("njobs", [1, 2, 17])
def test_batch_every_case(matcher, gpu, njobs):
    cases = sc.all_cases()
    groups = [cases[i:i + njobs] for i in range(0, len(cases), njobs)]
    assert any(len(g) == njobs for g in groups)
    for g in groups:
        if len(g) == njobs:
            _run_group(matcher, gpu, g)


def test_refused_jobs_beside_good_ones(matcher, gpu):
    names = ["count_above_min", "sparse_i1", "random_19", "random_21", "random_63", "later_tie",
             "fix_scale_on", "random_20"]
    cases = [sc.case_named(n) for n in names]
    items = [(c,) + _setup(c)[1:] for c in cases]
    b = Batch(items, gpu)

    def edit(jobs, corr, tri):
        corr["octave1"][b.corr_off[1] + 3] = 8                 # job 1: an octave == nlevels
        corr["i1"][b.corr_off[2] + 5] = cases[2]["mN1"]        # job 2: i1 == mN1
        tri[b.tri_off[3], 1] = tri[b.tri_off[3], 0]            # job 3: a repeated index
        jobs["corr_off"][5] = len(corr)                        # job 5: outside the array
        jobs["nlevels2"][6] = 17                               # job 6: nlevels above 16
        return jobs, corr, tri

    n_it = [c["calls"][0] for c in cases]
    # max_n below job 4's N (63): that job is refused for the limit
    res, inl, state = b.call(matcher, n_it, max_n=40, max_call=300, edit=edit)
    want = {1: SIM3_REFUSED_OCTAVE, 2: SIM3_REFUSED_I1, 3: SIM3_REFUSED_TRIPLE,
            4: SIM3_REFUSED_LIMIT, 5: SIM3_REFUSED_RANGE, 6: SIM3_REFUSED_OCTAVE}
    for j, c in enumerate(cases):
        if j in want:
            rec = _sentinel(1, SIM3_RESULT_DTYPE)
            rec["found"], rec["info"] = 0, want[j]
            assert res[j:j + 1].tobytes() == rec.tobytes(), (j, res[j])
            assert (inl[j] == S).all()
            assert (int(state[j]["iterations"]), int(state[j]["best_inliers"])) == c["state0"]
        else:
            call = sc.reference(c)["calls"][0]
            assert sc.canon(res[j:j + 1].tobytes()) == sc.canon(sc.result_record(call).tobytes()), j
            assert inl[j].tobytes() == call["inliers"].tobytes()
    # a triple index == N, and a job whose iterations exceed max_call_its
    b2 = Batch(items[:2], gpu)

    def edit2(jobs, corr, tri):
        tri[b2.tri_off[0] + 1, 2] = len(cases[0]["corr"])
        return jobs, corr, tri
    res, inl, _ = b2.call(matcher, [5, 30], max_call=5, edit=edit2)
    assert int(res[0]["info"]) == SIM3_REFUSED_TRIPLE and int(res[1]["info"]) == SIM3_REFUSED_LIMIT
    assert not res["found"].any() and (inl[0] == S).all() and (inl[1] == S).all()


def test_limits(matcher, gpu):
    lim = sim3_limits()
    c = sc.case_named("random_3")
    r, max_its, tri = _setup(c)
    call = sc.reference(c)["calls"][0]
    want = sc.canon(sc.result_record(call).tobytes())
    # the last supported sizes, each with the others small
    for kw in (dict(max_n=lim["max_n"]), dict(max_call=lim["max_its"])):
        res, inl, _ = Batch([(c, max_its, tri)], gpu).call(matcher, [c["calls"][0]], **kw)
        assert sc.canon(res.tobytes()) == want and inl[0].tobytes() == call["inliers"].tobytes()
    # the first: no correspondence at all (N < min_inliers) and iterate(0)
    empty = dict(c, corr=c["corr"][:0], mN1=0, name="empty")
    res, _, state = Batch([(empty, 1, np.zeros((1, 3), np.int32))], gpu).call(
        matcher, [0], max_n=0, max_call=0)
    assert res[0]["info"] == 0, hex(res[0]["info"])
    assert res[0]["no_more"] == 1 and res[0]["found"] == 0
    assert int(state[0]["iterations"]) == 0
    # the largest job count: the same small job max_jobs times over
    import torch
    n = lim["max_jobs"]
    jobs = np.zeros(n, SIM3_JOB_DTYPE)
    jobs[:] = sc.job_of(c, max_its, c["calls"][0], kf1=0, kf2=1)
    jobs["inlier_off"] = np.arange(n) * c["mN1"]
    dev = lambda a: torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).to(gpu)
    poses = np.stack([np.asarray(c[k], FRAME_POSE_DTYPE).reshape(()) for k in ("pose1", "pose2")])
    d_res, d_inl = dev(_sentinel(n, SIM3_RESULT_DTYPE)), dev(np.full(n * c["mN1"], S, np.uint8))
    d_state = dev(np.zeros(n, SIM3_STATE_DTYPE))
    args = [dev(jobs), n, 3, 1, dev(poses), dev(c["corr"]), dev(tri), d_state, d_res, d_inl]
    matcher.sim3_iterate_batch_device(*args)
    matcher.sync()
    res = np.frombuffer(d_res.cpu().numpy().tobytes(), SIM3_RESULT_DTYPE)
    assert sc.canon(res[:1].tobytes()) == want and res.tobytes() == res[:1].tobytes() * n
    assert d_inl.cpu().numpy().tobytes() == call["inliers"].tobytes() * n
    # one past each
    from my_orb_slam2_amd import OrbxError
    for k, v in ((1, n + 1), (2, lim["max_n"] + 1), (3, lim["max_its"] + 1)):
        a = list(args)
        a[k] = v
        with pytest.raises(OrbxError) as e:
            matcher.sim3_iterate_batch_device(*a)
        assert e.value.code == -4
    assert sim3_iterate(c["pose1"], c["pose2"], sc.job_of(c, max_its, 1), c["corr"], tri,
                        np.zeros(1, SIM3_STATE_DTYPE))[0]["info"] == 0


def test_solver_class_find_and_repeated_iterate(orbx_lib, gpu):
    """Sim3Solver by the reference's names: iterate(5) repeatedly against one find()."""
    c = sc.case_named("random_129")
    a = Sim3Solver(c["pose1"], c["pose2"], c["corr"], c["sigma2_1"], c["sigma2_2"], c["mN1"],
                   c["fix_scale"], c["rand"])
    a.SetRansacParameters(c["prob"], c["min_inliers"], c["max_iterations"])
    T, inl, n = a.find()
    want = sc.solve(dict(c, calls=(a.max_its,)))["calls"][0]
    assert want["found"] and n == want["n_inliers"]
    assert np.array_equal(inl, want["inliers"].astype(bool))
    assert T.tobytes() == sc.result_record(want)["T12"][0].tobytes()
    b = Sim3Solver(c["pose1"], c["pose2"], c["corr"], c["sigma2_1"], c["sigma2_2"], c["mN1"],
                   c["fix_scale"], c["rand"])
    b.SetRansacParameters(c["prob"], c["min_inliers"], c["max_iterations"])
    for _ in range(60):
        T5, no_more, inl5, n5 = b.iterate(5)
        if T5 is not None or no_more:
            break
    assert T5.tobytes() == T.tobytes() and n5 == n and np.array_equal(inl5, inl)
    assert b.GetEstimatedRotation().tobytes() == want["model"]["R"].tobytes()
    assert b.GetEstimatedTranslation().tobytes() == want["model"]["t"].tobytes()
    assert b.GetEstimatedScale() == float(want["model"]["s"])


def test_chain_bow_solver_projection_search(oracle_mod, orbx_lib, gpu):
    """SearchByBoW(KF, KF) -> Sim3Solver -> the SIM3 projections both ways -> SearchBySim3, the
    device results against the oracle's searches fed by the restatement's model."""
    from oracle import matcher as om
    from my_orb_slam2_amd import ORBmatcher
    f1, f2, truth = synth.feature_pair(91, n1=500, n2=480)
    rng = np.random.default_rng(91)
    v1, v2 = rng.random(f1.n) < 0.9, rng.random(f2.n) < 0.9
    m = ORBmatcher(0.75, True)
    n_g, m12 = m.SearchByBoW(f1, v1, f2, v2, f_is_keyframe=True)
    n_o, m12_o = om.search_by_bow_kf_kf(f1, v1, f2, v2, 0.75, True)
    assert n_g == n_o and n_o > 30
    np.testing.assert_array_equal(m12, m12_o)
    # the MapPoints behind the matches: a rigid transform between the two keyframes' frames
    # (mbFixScale, the stereo / RGB-D loop closer), displaced where the match is a wrong one
    K4, bounds = synth.EUROC_CAM[0], (0.0, 752.0, 0.0, 480.0)
    sf, s2, _ = synth.scale_tables()
    pose1, pose2 = pc.random_pose(92, K4, bounds), pc.random_pose(93, K4, bounds)
    i1 = np.flatnonzero(m12 >= 0)
    good = m12[i1] == truth[i1]
    assert good.sum() > 20
    X2c = np.stack([rng.uniform(-2, 2, len(i1)), rng.uniform(-1.5, 1.5, len(i1)),
                    rng.uniform(3, 8, len(i1))], 1)
    R12, t12 = sc.rodrigues64((0.2, -0.1, 0.3)), np.array([0.4, -0.2, 0.1])
    X1c = X2c @ R12.T + t12
    X1c[~good] += rng.uniform(-1, 1, ((~good).sum(), 3))
    P = lambda p: (p["Rcw"].reshape(3, 3).astype(np.float64), p["tcw"].astype(np.float64))
    (R1, t1), (R2, t2) = P(pose1), P(pose2)
    corr = np.zeros(len(i1), SIM3_CORR_DTYPE)
    corr["i1"] = i1
    corr["X1w"], corr["X2w"] = ((X1c - t1) @ R1).astype(np.float32), ((X2c - t2) @ R2).astype(np.float32)
    corr["octave1"], corr["octave2"] = f1.keys["octave"][i1], f2.keys["octave"][m12[i1]]
    rand = rng.integers(0, 2 ** 31, 900).astype(np.int32)
    case = dict(name="chain", pose1=pose1, pose2=pose2, sigma2_1=s2, sigma2_2=s2, corr=corr,
                mN1=f1.n, fix_scale=True, min_inliers=20, max_iterations=300, prob=0.99, rand=rand,
                calls=(300,), state0=(0, 0))
    want = sc.solve(case)["calls"][0]
    solver = Sim3Solver(pose1, pose2, corr, s2, s2, f1.n, True, rand)
    solver.SetRansacParameters(0.99, 20, 300)
    T, inl, n = solver.find()
    assert want["found"] and n == want["n_inliers"] >= good.sum() - 2
    assert np.array_equal(inl, want["inliers"].astype(bool))
    R, t, s = solver.GetEstimatedRotation(), solver.GetEstimatedTranslation(), solver.GetEstimatedScale()
    H = want["model"]
    assert R.tobytes() == H["R"].tobytes() and t.tobytes() == H["t"].tobytes() and s == 1.0
    # ORBmatcher::SearchBySim3's transforms (ORBmatcher.cc:1108-1117) from the device's model
    sR12 = (np.float32(s) * R).astype(np.float32)
    sR21 = ((np.float32(1.0) / np.float32(s)) * R.T).astype(np.float32)
    t21 = (-(sR21.astype(np.float64) @ t.astype(np.float64))).astype(np.float32)
    inv = np.full(f2.n, -1, np.int64)
    inv[truth[truth >= 0]] = np.nonzero(truth >= 0)[0]

    def one_way(seed, Rs, ts, pre, K_pose, f_dst, target):
        cam = frame_pose(Rs, ts, K4, bounds, sf)
        job = proj_job(cam, 7.5, pre["Rcw"].reshape(3, 3), pre["tcw"])
        Rp, tp = P(pre)
        whole = frame_pose(Rs.astype(np.float64) @ Rp, Rs.astype(np.float64) @ tp + ts, K4, bounds, sf)
        mps = pc.mappoints_onto(seed, whole, f_dst.keys, target)
        q_np, n_np, _ = pc.project_np(PROJ_SIM3, job, mps)
        q_gpu, n_gpu = project_map_points(PROJ_SIM3, job, mps)
        assert n_gpu == n_np and n_np > 0.8 * len(mps)
        assert q_gpu.tobytes() == q_np.tobytes()
        return q_gpu, q_np
    q12_g, q12_n = one_way(94, sR21, t21, pose1, pose2, f2, truth)     # KF1's MapPoints into KF2
    q21_g, q21_n = one_way(95, sR12, t, pose2, pose1, f1, inv)         # KF2's MapPoints into KF1
    n_g, m_g = m.SearchBySim3(f1, f2, f1.desc, q12_g, f2.desc, q21_g)
    n_o, m_o = om.search_by_sim3(f1, f2, f1.desc, q12_n, f2.desc, q21_n)
    assert n_g == n_o and n_o > 50
    np.testing.assert_array_equal(m_g, m_o)
