"""GPU: orbx_pnp_iterate / orbx_pnp_iterate_batch_device (k_pnp_hypotheses, k_pnp_select) bit for
bit against the Python restatement of tests/pnp_cases.py (which tests/test_pnp_cases.py holds
against the C++ restatement on the CPU), with sentinels in and around every output; refused jobs
beside good ones; the limits; orbx_pnp_correspondences_batch_device and orbx_pnp_apply_batch_device
against numpy; and the chain SearchByBoW(KF, Frame) -> correspondences -> PnPsolver -> apply ->
PoseOptimization with no host copy of matches or poses between the steps, against the same chain
with the restatement in the middle and against the generating pose."""
import numpy as np
import pytest

import pnp_cases as pc
from my_orb_slam2_amd import KEYPOINT_DTYPE, synth
from my_orb_slam2_amd.features import (FRAME_POSE_DTYPE, MAP_POINT_DTYPE, frame_pose,
                                       pose_optimization, pose_optimization_batch_device)
from my_orb_slam2_amd.pnp import (PNP_CORR_DTYPE, PNP_JOB_DTYPE, PNP_REFUSED_I, PNP_REFUSED_LIMIT,
                                  PNP_REFUSED_OCTAVE, PNP_REFUSED_QUAD, PNP_REFUSED_RANGE,
                                  PNP_RESULT_DTYPE, PNP_STATE_DTYPE, pnp_iterate, pnp_job,
                                  pnp_limits, pnp_ransac_parameters, pnp_sample_quads, pnp_window)
from test_pnp_cases import R_BOUND, T_BOUND

pytestmark = pytest.mark.gpu
S = pc.SENTINEL
GUARD = 64                      # sentinel bytes between the jobs' byte blocks
f32 = np.float32


def _sentinel(n, dtype):
    return np.frombuffer(bytes([S]) * (n * dtype.itemsize), dtype).copy()


def _state0(case):
    s = np.zeros(1, PNP_STATE_DTYPE)
    s["iterations"], s["best_inliers"] = case["state0"]
    s["best_Tcw"] = case["best_Tcw0"]
    return s


def _setup(case):
    """min_inliers, max_its and the quads through the library's own helpers."""
    N = len(case["corr"])
    r = pc.reference(case)
    mi, mx = pnp_ransac_parameters(case["prob"], case["min_inliers"], case["max_iterations"], 4,
                                   case["epsilon"], N)
    assert (mi, mx) == (r["min_inliers"], r["max_its"])
    q = pnp_sample_quads(N, case["rand"]) if N >= 4 else np.zeros((len(case["rand"]) // 4, 4),
                                                                  np.int32)
    for k, v in case["quad_edits"].items():
        q[k] = v
    assert np.array_equal(q, r["quads"])
    return r, mi, mx, q


def _same(res, inl, state, best, case, call, what):
    assert pc.canon(res.tobytes()) == pc.canon(pc.result_record(call).tobytes()), \
        (what, res, pc.result_record(call))
    assert inl.tobytes() == pc.expected_inliers(case, call).tobytes(), what
    assert pc.canon(state.tobytes()) == pc.canon(pc.state_record(call).tobytes()), \
        (what, state, pc.state_record(call))
    assert best.tobytes() == call["best"].tobytes(), what


def test_host_form_every_case(orbx_lib, gpu):
    assert {len(c["corr"]) for c in pc.all_cases()} >= {4, 10, 15, 40, 64, 65, 130}
    for c in pc.all_cases():
        r, mi, mx, q = _setup(c)
        state, best = _state0(c), c["best0"].copy()
        for k, (n_it, call) in enumerate(zip(c["calls"], r["calls"])):
            res = _sentinel(1, PNP_RESULT_DTYPE)
            inl = np.full(c["n_matches"], S, np.uint8)
            pnp_iterate(pc.job_of(c, mi, mx, n_it), c["corr"], q, state, best, res, inl)
            _same(res, inl, state, best, c, call, (c["name"], k))


def test_solver_class_follows_the_reference_surface(orbx_lib, gpu):
    """PnPsolver from a frame's arrays: its correspondences, its rand cursor (4 per executed
    iteration) and find() on an exact scene; fewer valid matches than mRansacMinInliers give
    bNoMore and nothing else."""
    for name in ("exact_40", "n_below_min"):
        c = pc.case_named(name)
        s = pc.solver_of(c)
        for n_it, call in zip(c["calls"], pc.reference(c)["calls"]):
            before = s.cursor
            T, no_more, inl, n = s.iterate(n_it)
            assert s.cursor - before == 4 * call["n_run"]
            assert (T is not None) == bool(call["found"]) and no_more == bool(call["no_more"])
            assert n == call["n_inliers"]
            if call["found"]:
                assert np.array_equal(T.reshape(16), call["Tcw"])
                assert np.array_equal(inl.astype(np.uint8), call["inliers"])
            else:
                assert inl.shape == (c["n_matches"],) and not inl.any()
    c = pc.case_named("exact_40")
    T, inl, n = pc.solver_of(c).find()
    f = pc.find(c)
    assert n == f["n_inliers"] == 40 and np.array_equal(T.reshape(16), f["Tcw"])
    assert np.abs(T[:3, :3] - c["R"]).max() <= R_BOUND and np.abs(T[:3, 3] - c["t"]).max() <= T_BOUND
    # a handful of matches under the class defaults (8, 0.4), N < 4 and N == 0 included, with no
    # rand() value at all: (None, bNoMore, no inlier, 0) from iterate, from a second iterate and
    # from find
    below = pc.case_named("n_below_min")
    for N in (7, 3, 0):
        s = pc.solver_of(dict(below, corr=below["corr"][:N], rand=np.zeros(0, np.int32)),
                    parameters=False)
        assert s.N == N < s.min_inliers == 8
        for _ in range(2):
            T, no_more, inl, n = s.iterate(5)
            assert T is None and no_more and n == 0 and s.cursor == 0
            assert inl.shape == (below["n_matches"],) and not inl.any()
            assert s.state.tobytes() == np.zeros(1, PNP_STATE_DTYPE).tobytes() and not s.best.any()
        T, inl, n = s.find()
        assert T is None and n == 0 and not inl.any()


class Batch:
    """The device arrays of one batched call over `items` = [(case, min_inliers, max_its, quads)],
    each job with its own slice of every array and sentinels between and around them."""

    def __init__(self, items, gpu):
        import torch
        self.items, self.gpu, self.torch = items, gpu, torch
        self.n = len(items)
        self.corr = np.concatenate([c["corr"] for c, _, _, _ in items] + [np.zeros(1, PNP_CORR_DTYPE)])
        self.quads = np.concatenate([q.reshape(-1, 4) for _, _, _, q in items]).astype(np.int32)
        self.corr_off = np.cumsum([0] + [len(c["corr"]) for c, _, _, _ in items])
        self.quad_off = np.cumsum([0] + [len(q) for _, _, _, q in items])
        self.inl_off = np.cumsum([GUARD] + [c["n_matches"] + GUARD for c, _, _, _ in items])
        self.best_off = np.cumsum([GUARD] + [len(c["corr"]) + GUARD for c, _, _, _ in items])
        self.state = _sentinel(self.n + 2, PNP_STATE_DTYPE)
        self.best = np.full(int(self.best_off[-1]), S, np.uint8)
        for j, (c, _, _, _) in enumerate(items):
            self.state[j + 1] = _state0(c)[0]
            self.best[self.best_off[j]:self.best_off[j] + len(c["corr"])] = c["best0"]

    def dev(self, a):
        return self.torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).to(self.gpu)

    def call(self, matcher, n_iterations, max_n=None, max_call=None, edit=None):
        """One iterate(n_iterations[j]) of every job -> (results, inlier bytes, states, best)."""
        jobs = np.zeros(self.n, PNP_JOB_DTYPE)
        windows = []
        for j, (c, mi, mx, _) in enumerate(self.items):
            jobs[j] = pc.job_of(c, mi, mx, n_iterations[j], corr_off=self.corr_off[j],
                                inlier_off=self.inl_off[j], quad_off=self.quad_off[j],
                                best_off=self.best_off[j])
            windows.append(pnp_window(mx, self.state[j + 1]["iterations"], n_iterations[j]))
        corr, quads = self.corr, self.quads
        if edit:
            jobs, corr, quads = edit(jobs, corr.copy(), quads.copy())
        max_n = max(len(c["corr"]) for c, _, _, _ in self.items) if max_n is None else max_n
        max_call = max(windows) if max_call is None else max_call
        res = _sentinel(self.n + 2, PNP_RESULT_DTYPE)
        inl = np.full(int(self.inl_off[-1]), S, np.uint8)
        d_jobs, d_corr, d_quads = self.dev(jobs), self.dev(corr), self.dev(quads)
        d_state, d_best, d_res, d_inl = (self.dev(a) for a in (self.state, self.best, res, inl))
        si, ri = PNP_STATE_DTYPE.itemsize, PNP_RESULT_DTYPE.itemsize
        matcher.pnp_iterate_batch_device(d_jobs, self.n, max_n, max_call, d_corr, d_quads,
                                         d_state[si:-si], d_best, d_res[ri:-ri], d_inl)
        matcher.sync()
        res = np.frombuffer(d_res.cpu().numpy().tobytes(), PNP_RESULT_DTYPE)
        inl, best = d_inl.cpu().numpy(), d_best.cpu().numpy()
        state = np.frombuffer(d_state.cpu().numpy().tobytes(), PNP_STATE_DTYPE).copy()
        # the guards around the results and the states, and between the byte blocks
        assert res[[0, -1]].tobytes() == bytes([S]) * (2 * ri)
        assert state[[0, -1]].tobytes() == bytes([S]) * (2 * si)
        for j in range(self.n + 1):
            assert (inl[self.inl_off[j] - GUARD:self.inl_off[j]] == S).all()
            assert (best[self.best_off[j] - GUARD:self.best_off[j]] == S).all()
        self.state, self.best = state, best.copy()
        return (res[1:-1],
                [inl[self.inl_off[j]:self.inl_off[j] + c["n_matches"]]
                 for j, (c, _, _, _) in enumerate(self.items)], state[1:-1],
                [best[self.best_off[j]:self.best_off[j] + len(c["corr"])]
                 for j, (c, _, _, _) in enumerate(self.items)])


@pytest.fixture(scope="module")
def matcher(orbx_lib, gpu):
    from my_orb_slam2_amd import ORBmatcher
    return ORBmatcher(0.75, True)


def _run_group(matcher, gpu, cases):
    items = [(c,) + _setup(c)[1:] for c in cases]
    refs = [pc.reference(c)["calls"] for c in cases]
    b = Batch(items, gpu)
    for k in range(max(len(c["calls"]) for c in cases)):
        live = [j for j, c in enumerate(cases) if k < len(c["calls"])]
        # a job whose case has no k-th call would run again under `||`: give it to a fresh batch
        sub = Batch([items[j] for j in live], gpu)
        for a, j in enumerate(live):
            sub.state[a + 1] = b.state[j + 1]
            n = len(cases[j]["corr"])
            sub.best[sub.best_off[a]:sub.best_off[a] + n] = b.best[b.best_off[j]:b.best_off[j] + n]
        res, inl, state, best = sub.call(matcher, [cases[j]["calls"][k] for j in live])
        for a, j in enumerate(live):
            _same(res[a:a + 1], inl[a], state[a:a + 1], best[a], cases[j], refs[j][k],
                  (cases[j]["name"], k))
            b.state[j + 1] = state[a]
            n = len(cases[j]["corr"])
            b.best[b.best_off[j]:b.best_off[j] + n] = best[a]


@pytest.mark.parametrize("njobs", [1, 3, 8])
def test_batch_every_case(matcher, gpu, njobs):
    """Mixed sizes in one call, the state and the best bytes carried over up to three calls."""
    cases = pc.all_cases()
    assert max(len(c["calls"]) for c in cases) == 3
    groups = [cases[i:i + njobs] for i in range(0, len(cases), njobs)]
    for g in groups:
        _run_group(matcher, gpu, list(g))


def test_refused_jobs_beside_good_ones(matcher, gpu):
    names = ["exact_10", "exact_15", "exact_40", "outliers_40", "exact_64", "equal_z_quad",
             "returned_then_again", "n_is_4"]
    cases = [pc.case_named(n) for n in names]
    items = [(c,) + _setup(c)[1:] for c in cases]
    b = Batch(items, gpu)

    def edit(jobs, corr, quads):
        corr["octave"][b.corr_off[1] + 3] = 8                   # job 1: an octave == nlevels
        corr["i"][b.corr_off[2] + 5] = corr["i"][b.corr_off[2] + 4]   # job 2: i not increasing
        quads[b.quad_off[3], 1] = quads[b.quad_off[3], 0]       # job 3: a repeated index
        jobs["corr_off"][5] = len(corr)                         # job 5: outside the array
        jobs["nlevels"][6] = 17                                 # job 6: nlevels above 16
        return jobs, corr, quads

    n_it = [c["calls"][0] for c in cases]
    # max_n below job 4's N (64): that job is refused for the limit
    res, inl, state, best = b.call(matcher, n_it, max_n=40, max_call=35, edit=edit)
    want = {1: PNP_REFUSED_OCTAVE, 2: PNP_REFUSED_I, 3: PNP_REFUSED_QUAD, 4: PNP_REFUSED_LIMIT,
            5: PNP_REFUSED_RANGE, 6: PNP_REFUSED_OCTAVE}
    for j, c in enumerate(cases):
        if j in want:
            rec = _sentinel(1, PNP_RESULT_DTYPE)
            rec["found"], rec["info"] = 0, want[j]
            assert res[j:j + 1].tobytes() == rec.tobytes(), (j, res[j])
            assert (inl[j] == S).all() and best[j].tobytes() == c["best0"].tobytes()
            assert state[j:j + 1].tobytes() == _state0(c).tobytes()
        else:
            call = pc.reference(c)["calls"][0]
            _same(res[j:j + 1], inl[j], state[j:j + 1], best[j], c, call, j)
    # an index == N, an i == n_matches, a window above max_call_its, a state that contradicts its
    # best bytes, min_inliers < 1
    b2 = Batch(items[:5], gpu)
    b2.state[5]["best_inliers"] = 3

    def edit2(jobs, corr, quads):
        quads[b2.quad_off[0] + 1, 2] = len(cases[0]["corr"])
        corr["i"][b2.corr_off[1] + 14] = cases[1]["n_matches"]
        jobs["min_inliers"][3] = 0
        return jobs, corr, quads
    res, inl, _, _ = b2.call(matcher, [5, 5, 40, 5, 5], max_call=35, edit=edit2)
    assert [int(r["info"]) for r in res] == [PNP_REFUSED_QUAD, PNP_REFUSED_I, PNP_REFUSED_LIMIT,
                                             PNP_REFUSED_LIMIT, PNP_REFUSED_LIMIT]
    assert not res["found"].any() and all((x == S).all() for x in inl)


def test_limits_and_statuses(matcher, gpu):
    import torch
    L, h = matcher._lib, matcher._h
    lim = pnp_limits()
    z = torch.zeros(4096, dtype=torch.uint8, device=gpu)
    p = z.data_ptr()

    def batch(njobs=1, max_n=8, max_call=8, jobs=p, corr=p, quads=p, state=p, best=p, res=p, inl=p,
              ncorr=8, nquads=8, nbest=8, ninl=8, m=h):
        return L.orbx_pnp_iterate_batch_device(m, jobs, njobs, max_n, max_call, corr, ncorr, quads,
                                               nquads, state, best, nbest, res, inl, ninl, None)
    for kw in (dict(m=None), dict(njobs=-1), dict(max_n=-1), dict(max_call=-1), dict(ncorr=-1),
               dict(nquads=-1), dict(nbest=-1), dict(ninl=-1), dict(jobs=None), dict(state=None),
               dict(res=None), dict(corr=None), dict(quads=None), dict(best=None), dict(inl=None)):
        assert batch(**kw) == -1, kw
    assert batch(njobs=0, jobs=None, state=None, res=None) == 0
    assert batch(njobs=lim["max_jobs"] + 1) == -4
    assert batch(max_n=lim["max_n"] + 1) == -4
    assert batch(max_call=lim["max_its"] + 1) == -4
    # within each limit, but the scratch of the three together is above the bound
    assert batch(njobs=lim["max_jobs"], max_n=lim["max_n"], max_call=lim["max_its"]) == -4
    matcher.sync()
    assert (z == 0).all()


# ---- the two kernels around the solver -----------------------------------------------------------

def _np_correspondences(match_row, keys, mps):
    idx = np.flatnonzero((match_row >= 0) & (match_row < len(mps)))
    c = np.zeros(len(idx), PNP_CORR_DTYPE)
    c["i"], c["X"] = idx, mps["pos"][match_row[idx]]
    c["u"], c["v"], c["octave"] = keys["x"][idx], keys["y"][idx], keys["octave"][idx]
    return c


def _np_apply(tmpl, call_found, Tcw, inliers, match_row):
    P = np.array(tmpl, FRAME_POSE_DTYPE).reshape(1).copy()
    if not call_found:
        return P, np.full(len(match_row), -1, np.int32)
    T = np.asarray(Tcw, f32).reshape(4, 4)
    R, t = T[:3, :3], T[:3, 3]
    P["Rcw"], P["tcw"] = R.reshape(9), t
    for a in range(3):
        acc = f32(R[0, a] * t[0])
        acc = f32(acc + f32(R[1, a] * t[1]))
        acc = f32(acc + f32(R[2, a] * t[2]))
        P["Ow"][0, a] = -acc
    return P, np.where(np.asarray(inliers) != 0, match_row, -1).astype(np.int32)


def test_correspondences_and_apply_against_numpy(matcher, gpu):
    import torch
    rng = np.random.default_rng(9)
    # n_feat on both sides of the 256-thread pass, and empty
    for n_feat, njobs in ((0, 2), (1, 1), (255, 3), (256, 2), (257, 2), (700, 4)):
        stride = n_feat + 5
        nmp = [int(rng.integers(1, 300)) for _ in range(njobs)]
        mp_off = np.cumsum([0] + nmp).astype(np.int32)
        mps = np.zeros(mp_off[-1], MAP_POINT_DTYPE)
        mps["pos"] = rng.normal(size=(len(mps), 3)).astype(f32)
        keys = np.zeros(max(n_feat, 1), KEYPOINT_DTYPE)[:n_feat]
        keys["x"], keys["y"] = rng.uniform(0, 640, n_feat), rng.uniform(0, 480, n_feat)
        keys["octave"] = rng.integers(0, 8, n_feat)
        match = np.full((njobs, stride), -1, np.int32)
        for j in range(njobs):
            row = rng.integers(0, nmp[j], n_feat)
            row[rng.random(n_feat) < 0.6] = -1
            if n_feat > 3 and j == 0:
                row[3] = nmp[j]                # outside the block: dropped and flagged
            match[j, :n_feat] = row
        dev = lambda a: torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).to(gpu)
        d_corr = dev(_sentinel(njobs * stride + 1, PNP_CORR_DTYPE))
        d_N, d_fl = dev(np.full(njobs + 1, -9, np.int32)), dev(np.full(njobs + 1, -9, np.int32))
        matcher.pnp_correspondences_batch_device(njobs, dev(match), stride, dev(keys), n_feat,
                                                 dev(mps), dev(mp_off), d_corr, stride, d_N, d_fl)
        matcher.sync()
        corr = np.frombuffer(d_corr.cpu().numpy().tobytes(), PNP_CORR_DTYPE)
        N = np.frombuffer(d_N.cpu().numpy().tobytes(), np.int32)
        fl = np.frombuffer(d_fl.cpu().numpy().tobytes(), np.int32)
        assert N[-1] == -9 and fl[-1] == -9
        sent = _sentinel(1, PNP_CORR_DTYPE).tobytes()
        for j in range(njobs):
            want = _np_correspondences(match[j, :n_feat], keys, mps[mp_off[j]:mp_off[j + 1]])
            assert N[j] == len(want) and fl[j] == int(n_feat > 3 and j == 0)
            got = corr[j * stride:(j + 1) * stride]
            assert got[:N[j]].tobytes() == want.tobytes(), (n_feat, j)
            assert all(g.tobytes() == sent for g in got[N[j]:])
        assert corr[-1].tobytes() == sent

        # apply: found, not found, refused, and a job whose n_matches is not n_feat
        jobs = np.zeros(njobs, PNP_JOB_DTYPE)
        res = np.zeros(njobs, PNP_RESULT_DTYPE)
        inl = (rng.random(njobs * (n_feat + GUARD) + GUARD) < 0.5).astype(np.uint8)
        for j in range(njobs):
            jobs[j]["n_matches"] = n_feat if j != 3 else n_feat + 1
            jobs[j]["inlier_off"] = GUARD + j * (n_feat + GUARD)
            res[j]["found"] = int(j != 1)
            res[j]["Tcw"] = rng.normal(size=16).astype(f32)
            if j == 2:
                res[j]["info"] = PNP_REFUSED_I
        tmpl = frame_pose(np.eye(3), np.zeros(3), pc.K4, (0, 640, 0, 480), synth.scale_tables()[0])
        d_poses = dev(_sentinel(njobs + 1, FRAME_POSE_DTYPE))
        d_mpf = dev(np.full(njobs * stride + 1, -9, np.int32))
        matcher.pnp_apply_batch_device(njobs, dev(jobs), dev(res), dev(inl), dev(match), stride,
                                       n_feat, dev(np.asarray(tmpl)), d_poses, d_mpf, stride)
        matcher.sync()
        poses = np.frombuffer(d_poses.cpu().numpy().tobytes(), FRAME_POSE_DTYPE)
        mpf = np.frombuffer(d_mpf.cpu().numpy().tobytes(), np.int32)
        assert poses[-1].tobytes() == _sentinel(1, FRAME_POSE_DTYPE).tobytes() and mpf[-1] == -9
        for j in range(njobs):
            found = j not in (1, 2, 3)
            o = int(jobs[j]["inlier_off"])
            P, m = _np_apply(tmpl, found, res[j]["Tcw"], inl[o:o + n_feat], match[j, :n_feat])
            assert poses[j:j + 1].tobytes() == P.tobytes(), (n_feat, j)
            assert np.array_equal(mpf[j * stride:j * stride + n_feat], m)
            assert (mpf[j * stride + n_feat:(j + 1) * stride] == -9).all()


# ---- the chain --------------------------------------------------------------------------------------

def test_chain_bow_pnp_poseopt_without_host_copies(matcher, gpu):
    import torch
    from my_orb_slam2_amd.matcher import DeviceFeatureSet, DeviceKfDb
    frame, R, t, kfs, valids, mps = pc.small_map(300)
    K, nf = len(kfs), frame.n
    scale, sigma2, _ = synth.scale_tables()
    dev = lambda a: torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy()).to(gpu)
    db, df = DeviceKfDb(kfs, valids, gpu), DeviceFeatureSet(frame, gpu)
    mp_off = np.cumsum([0] + [len(m) for m in mps]).astype(np.int32)
    d_mps, d_mp_off = dev(np.concatenate(mps)), dev(mp_off)
    d_match = torch.full((K, nf), -7, dtype=torch.int32, device=gpu)
    d_cnt = torch.zeros(K, dtype=torch.int32, device=gpu)
    d_corr = dev(np.zeros(K * nf, PNP_CORR_DTYPE))
    d_N = torch.zeros(K, dtype=torch.int32, device=gpu)
    matcher.search_by_bow_kf_frame_batch_device(db.c, df.c, d_match, d_cnt)
    matcher.pnp_correspondences_batch_device(K, d_match, nf, df.keys, nf, d_mps, d_mp_off, d_corr, nf,
                                             d_N)
    matcher.sync()
    # what the caller reads back: the counts (the reference decides nmatches < 15 on the host)
    N = d_N.cpu().numpy()
    assert np.array_equal(N, d_cnt.cpu().numpy()) and (N[:3] >= 30).all() and N[3] < 10
    # Tracking.cc:1518: SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991); iterate(5) until a pose
    params = [pnp_ransac_parameters(0.99, 10, 300, 4, 0.5, int(n)) for n in N]
    rng = np.random.default_rng(4)
    n_q = 80
    rand = rng.integers(0, pc.RAND_MAX, size=(K, 4 * n_q), endpoint=True).astype(np.int32)
    quads = np.stack([pnp_sample_quads(int(N[j]), rand[j]) if N[j] >= 4 else
                      np.zeros((n_q, 4), np.int32) for j in range(K)])
    jobs = np.zeros(K, PNP_JOB_DTYPE)
    for j in range(K):
        jobs[j] = pnp_job(pc.K4, sigma2, 5.991, nf, int(N[j]), params[j][0], params[j][1], 5,
                          corr_off=j * nf, inlier_off=j * nf, quad_off=j * n_q, best_off=j * nf)
    d_jobs, d_quads = dev(jobs), dev(quads)
    d_state, d_best = dev(np.zeros(K, PNP_STATE_DTYPE)), dev(np.zeros(K * nf, np.uint8))
    d_res, d_inl = dev(np.zeros(K, PNP_RESULT_DTYPE)), dev(np.zeros(K * nf, np.uint8))
    window = max(pnp_window(p[1], 0, 5) for p in params)
    assert window <= 35
    matcher.pnp_iterate_batch_device(d_jobs, K, nf, window, d_corr, d_quads, d_state, d_best, d_res,
                                     d_inl)
    tmpl = frame_pose(np.eye(3), np.zeros(3), pc.K4, (0, 640, 0, 480), scale)
    d_poses = dev(np.zeros(K, FRAME_POSE_DTYPE))
    d_mpf = torch.full((K, nf), -5, dtype=torch.int32, device=gpu)
    matcher.pnp_apply_batch_device(K, d_jobs, d_res, d_inl, d_match, nf, nf, dev(np.asarray(tmpl)),
                                   d_poses, d_mpf, nf)
    # PoseOptimization reads frame j's features at [j * nf, (j + 1) * nf): the frame's keys once
    # per candidate
    d_keys = df.keys.repeat(K)
    d_feat_off = dev(np.arange(K + 1, dtype=np.int32) * nf)
    d_out = dev(np.zeros(K, FRAME_POSE_DTYPE))
    d_outlier = torch.zeros(K * nf, dtype=torch.uint8, device=gpu)
    d_ngood, d_info = (torch.zeros(K, dtype=torch.int32, device=gpu) for _ in range(2))
    pose_optimization_batch_device(d_poses, K, d_keys, None, d_feat_off, nf, d_mpf, d_mps, d_mp_off,
                                   d_out, d_outlier, d_ngood, d_info)
    matcher.sync()

    # the same chain with the restatement in the middle
    match = d_match.cpu().numpy()
    res = np.frombuffer(d_res.cpu().numpy().tobytes(), PNP_RESULT_DTYPE)
    out = np.frombuffer(d_out.cpu().numpy().tobytes(), FRAME_POSE_DTYPE)
    ngood = d_ngood.cpu().numpy()
    for j in range(K):
        corr = _np_correspondences(match[j], frame.keys, mps[j])
        assert len(corr) == N[j]
        state = dict(iterations=0, best_inliers=0, best_Tcw=np.zeros(16, f32))
        call = pc.iterate(jobs[j], corr, quads[j], state, np.zeros(len(corr), np.uint8))
        assert pc.canon(res[j:j + 1].tobytes()) == pc.canon(pc.result_record(call).tobytes()), j
        P, mpf = _np_apply(tmpl, call["found"], call["Tcw"], call["inliers"], match[j])
        po, _, ng, _ = pose_optimization(P[0], frame.keys, mpf, mps[j])
        assert out[j:j + 1].tobytes() == np.asarray(po).reshape(1).tobytes() and ngood[j] == ng, j
        if j < 3:
            assert call["found"] and ng >= 30
            Rr, tr = out[j]["Rcw"].reshape(3, 3).astype(np.float64), out[j]["tcw"].astype(np.float64)
            er, et = np.abs(Rr - R).max(), np.abs(tr - t).max()
            print(f"candidate {j}: N {N[j]}, nGood {ng}, R {er:.3e}, t {et:.3e}")
            assert er <= R_BOUND and et <= T_BOUND, (j, er, et)
        else:
            assert not call["found"] and ng == 0
            assert out[j:j + 1].tobytes() == np.asarray(tmpl).reshape(1).tobytes()
